"""Command line of src/main/wc.go (wc.go:40-58) over the GPU word count:

  python -m wcg.wc master <file> sequential          RunSingle(5, 3, ...) on the GPU
  python -m wcg.wc master <file> <master-socket>     MakeMapReduce(5, 3, ...), waits for workers
  python -m wcg.wc worker <master-socket> <me>       RunWorker(..., nRPC = 100) on the GPU
  python -m wcg.wc top <file> <N>                    the N most frequent words to stdout: what
                                                     `sort -n -k2 mrtmp.<file> | tail -<N>` prints
                                                     (test-wc.sh:2-3), selected on the GPU
  python -m wcg.wc count <file> <word>...            "<word>: <count>" per argument, in argument
                                                     order, zeros included, looked up on the GPU
  python -m wcg.wc prefix <file> <P>                 the merged file's lines whose key starts with P
  python -m wcg.wc by-count <file> [FIRST [N]]       the merged file in count order, what `sort -n -k2
                                                     mrtmp.<file>` prints, from line FIRST (default 0)
                                                     on, N lines (default: all), sorted on the GPU
  python -m wcg.wc at-least <file> <C>               its lines whose count is at least C, in that order
  python -m wcg.wc by-count-merged <mrtmp> [FIRST [N]]   the same two asked of a merged file that
  python -m wcg.wc at-least-merged <mrtmp> <C>           already exists
  python -m wcg.wc top-merged <mrtmp> <N>            the same three questions asked of a merged file
  python -m wcg.wc count-merged <mrtmp> <word>...    that already exists (mrtmp.<file>, ours or the
  python -m wcg.wc prefix-merged <mrtmp> <P>         CPU reference's): checked, loaded and searched
                                                     on the GPU, no input file and no re-run needed

nMap = 5, nReduce = 3 and nRPC = 100 are wc.go's constants (wc.go:49,51,56).  Environment knobs a
harness may set without changing that interface: WCG_DEVICE (HIP device of this process, default
0), WCG_NRPC (the worker's RPC budget, the failure-injection knob of worker.go:80-89),
WCG_JSON_INTERMEDIATES=1 (DoMap writes the reference's per-occurrence JSON -m-r files).

Device tables are sized from the input: a distinct key needs at least two input bytes (a letter
and a separator), so a job is first run with room for one key per 16 input bytes and, if the
aggregation table fills (WCG_EFULL), run again with room for every key the input could hold.
"""
from __future__ import annotations

import os
import sys

from . import mr

NMAP, NREDUCE, NRPC = 5, 3, 100           # wc.go:49, 51, 56
MAX_SPLIT = 1 << 30                       # parity domain P2: DoMap reads a split with one Read


def _device() -> int:
    return int(os.environ.get("WCG_DEVICE", "0"))


def _keys_for(nbytes: int, dense: bool) -> int:
    return max(1 << 18, nbytes // (2 if dense else 16) + 1024)


def engine_for(nbytes: int, dense: bool = False):
    """An engine whose tables hold the distinct keys of `nbytes` of input (dense: the worst case,
    one key per 2 bytes; else one per 16 bytes)."""
    from ._lib import Engine
    return Engine(device=_device(), max_input_bytes=min(max(nbytes, 1), MAX_SPLIT) + (64 << 10),
                  max_keys=_keys_for(nbytes, dense))


class SizedEngine:
    """Engine proxy for long-lived workers: ensure(nbytes, dense) re-opens the device context when
    a job needs larger tables or a larger staging buffer than the current one has (mr.py calls it
    before every job and again, dense, when a job's table filled)."""

    def __init__(self):
        self._e = None
        self._keys = self._staging = 0

    def ensure(self, nbytes: int, dense: bool = False) -> None:
        keys, staging = _keys_for(nbytes, dense), min(max(nbytes, 1 << 20), MAX_SPLIT)
        if self._e is None or keys > self._keys or staging > self._staging:
            if self._e is not None:
                self._e.close()
            from ._lib import Engine
            self._keys, self._staging = max(keys, self._keys), max(staging, self._staging)
            self._e = Engine(device=_device(), max_input_bytes=self._staging + (64 << 10), max_keys=self._keys)

    def __getattr__(self, name):
        if self._e is None:
            self.ensure(1 << 20)
        return getattr(self._e, name)

    def close(self):
        if self._e is not None:
            self._e.close()
            self._e = None


def run_single(path: str, nmap: int = NMAP, nreduce: int = NREDUCE) -> bytes:
    """RunSingle (mapreduce.go:344-356) on the GPU with tables sized from the input."""
    from ._lib import WcgError, WCG_EFULL
    workdir = os.path.dirname(os.path.abspath(path))
    size = os.path.getsize(path)
    for dense in (False, True):
        with engine_for(size, dense) as e:
            try:
                return mr.run_single(nmap, nreduce, path, e, workdir)
            except WcgError as err:
                if err.status != WCG_EFULL or dense:
                    raise
    raise AssertionError("unreachable")


def top(path: str, n: int = 10) -> bytes:
    """The n most frequent words of a file (test-wc.sh:2-3: `sort -n -k2 | tail -n`), selected on
    the GPU: Split + DoMap of the file (map_file, quirk P1 included), reduce, Engine.top.  Tables
    sized from the input as in run_single; writes no mrtmp.* files."""
    from ._lib import WcgError, WCG_EFULL
    size = os.path.getsize(path)
    for dense in (False, True):
        with engine_for(size, dense) as e:
            try:
                e.map_file(path)
                e.reduce()
                return e.top(n)
            except WcgError as err:
                if err.status != WCG_EFULL or dense:
                    raise
    raise AssertionError("unreachable")


def _reduced(path: str, query):
    """query(engine) after Split + DoMap + reduce of a file, as top() runs them"""
    from ._lib import WcgError, WCG_EFULL
    size = os.path.getsize(path)
    for dense in (False, True):
        with engine_for(size, dense) as e:
            try:
                e.map_file(path)
                e.reduce()
                return query(e)
            except WcgError as err:
                if err.status != WCG_EFULL or dense:
                    raise
    raise AssertionError("unreachable")


def count(path: str, words) -> list:
    """How often each of `words` (bytes) occurs in a file, 0 included, in the order asked: the
    counts its merged file gives them, looked up on the GPU (Engine.lookup); writes no mrtmp.* files."""
    words = list(words)
    return _reduced(path, lambda e: e.lookup(words))


def prefix(path: str, p: bytes) -> bytes:
    """The merged file's lines of a file whose key starts with p, selected on the GPU
    (Engine.prefix); writes no mrtmp.* files."""
    return _reduced(path, lambda e: e.prefix(p))


def _loaded(path: str, query):
    """query(engine) after Engine.load_merged of a merged file.  The engine is sized from the file's
    line count (its keys), not from an input size; the aggregation tables stay unused."""
    from ._lib import Engine
    with open(path, "rb") as f:
        data = f.read()
    with Engine(device=_device(), max_input_bytes=0, max_keys=max(1 << 16, data.count(b"\n"))) as e:
        e.load_merged(data)
        return query(e)


def top_merged(path: str, n: int = 10) -> bytes:
    """top() asked of a merged file: `sort -n -k2 <path> | tail -n <n>`, selected on the GPU."""
    return _loaded(path, lambda e: e.top(n))


def count_merged(path: str, words) -> list:
    """count() asked of a merged file: each word's count in it, 0 included, in the order asked."""
    words = list(words)
    return _loaded(path, lambda e: e.lookup(words))


def prefix_merged(path: str, p: bytes) -> bytes:
    """prefix() asked of a merged file: its lines whose key starts with p."""
    return _loaded(path, lambda e: e.prefix(p))


def by_count(path: str, first: int = 0, n=None) -> bytes:
    """The merged file of a file in count order (`sort -n -k2`), lines [first, first + n) of it
    (n = None: to the end), sorted on the GPU (Engine.by_count); writes no mrtmp.* files."""
    return _reduced(path, lambda e: e.by_count(first, n))


def at_least(path: str, c: int) -> bytes:
    """The merged file's lines of a file whose count is at least c, in count order (Engine.at_least)."""
    return _reduced(path, lambda e: e.at_least(c))


def by_count_merged(path: str, first: int = 0, n=None) -> bytes:
    """by_count() asked of a merged file."""
    return _loaded(path, lambda e: e.by_count(first, n))


def at_least_merged(path: str, c: int) -> bytes:
    """at_least() asked of a merged file."""
    return _loaded(path, lambda e: e.at_least(c))


def main(argv) -> int:
    if 3 <= len(argv) <= 5 and argv[1] in ("by-count", "by-count-merged"):
        fn = by_count if argv[1] == "by-count" else by_count_merged
        sys.stdout.buffer.write(fn(argv[2], int(argv[3]) if len(argv) > 3 else 0, int(argv[4]) if len(argv) > 4 else None))
        sys.stdout.buffer.flush()
        return 0
    if len(argv) >= 4 and argv[1] == "count-merged":
        words = [os.fsencode(w) for w in argv[3:]]
        out = b"".join(w + b": %d\n" % n for w, n in zip(words, count_merged(argv[2], words)))
        sys.stdout.buffer.write(out)
        sys.stdout.buffer.flush()
        return 0
    if len(argv) >= 4 and argv[1] == "count":
        words = [os.fsencode(w) for w in argv[3:]]
        out = b"".join(w + b": %d\n" % n for w, n in zip(words, count(argv[2], words)))
        sys.stdout.buffer.write(out)
        sys.stdout.buffer.flush()
        return 0
    if len(argv) != 4:                    # wc.go:45-46: a note, exit status 0
        print(f"{argv[0]}: see usage comments in file")
        return 0
    if argv[1] == "master":
        workdir = os.path.dirname(os.path.abspath(argv[2]))
        if argv[3] == "sequential":
            run_single(argv[2])
        else:
            mr.MapReduce(NMAP, NREDUCE, argv[2], argv[3], workdir).wait()
    elif argv[1] == "top":
        sys.stdout.buffer.write(top(argv[2], int(argv[3])))
        sys.stdout.buffer.flush()
    elif argv[1] == "at-least":
        sys.stdout.buffer.write(at_least(argv[2], int(argv[3])))
        sys.stdout.buffer.flush()
    elif argv[1] == "at-least-merged":
        sys.stdout.buffer.write(at_least_merged(argv[2], int(argv[3])))
        sys.stdout.buffer.flush()
    elif argv[1] == "top-merged":
        sys.stdout.buffer.write(top_merged(argv[2], int(argv[3])))
        sys.stdout.buffer.flush()
    elif argv[1] == "prefix-merged":
        sys.stdout.buffer.write(prefix_merged(argv[2], os.fsencode(argv[3])))
        sys.stdout.buffer.flush()
    elif argv[1] == "prefix":
        sys.stdout.buffer.write(prefix(argv[2], os.fsencode(argv[3])))
        sys.stdout.buffer.flush()
    else:
        nrpc = int(os.environ.get("WCG_NRPC", str(NRPC)))
        w = mr.Worker(argv[2], argv[3], SizedEngine, os.getcwd(), nrpc,
                      json_intermediates=os.environ.get("WCG_JSON_INTERMEDIATES") == "1").start()
        w.join()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
