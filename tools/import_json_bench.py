#!/usr/bin/env python3
"""Reading the reference's JSON files on the GPU: wcg_import_json_device against what a GPU DoReduce
and Merge had without it - decode the lines in Python, then count the keys on the GPU.

One job: a slice of a BASELINE corpus, its DoMap intermediates made by wcg_map_json for R
partitions (every line one occurrence) and its DoReduce -res files made by wcg_partition_all, all
resident on the device.  A second engine then, in one process and in turn per repetition:

  MAP   wcg_import_json_device of the R intermediate files, whole;
        the same with WCG_IMPORT_JSON_STOP=1 (the newline and checking passes only) and =2 (those and
        the write pass that compacts the keys; write = the difference, per repetition);
        wcg_map_device of the compacted "key\\n" text alone (what decoding adds is the rest);
        the parent's path on the same bytes: mr._json_keys on the host, then map_host (fewer
        repetitions: it takes seconds);
  RES   wcg_import_json_device of the R -res files; mr.merge_gpu and mr.merge from the files on disk.

A host clock around each group of calls (every one ends in a stream synchronise); medians with
minimum and maximum.  The bytes the passes must move (the text read by the newline, checking and
write pass, the key text written and read again by the map) over 8 TB/s stand next to it as the
floor.  Every answer is compared with the host's; a mismatch exits 3.

  python tools/import_json_bench.py [--mib 64] [--nreduce 4] [--reps 7] [--host-reps 3] [--warmup 2]
                                    [--out profiles/import_json_c2.json]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mit-6.824-2015_amd"))
sys.path.insert(0, ROOT)

CONFIG = "c2_ascii_zipf_1gib"
HBM_BYTES_PER_S = 8e12


def log(*a):
    print(f"[import_json_bench {time.strftime('%H:%M:%S')}]", *a, flush=True)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def clock(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--nreduce", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 2 and args.host_reps >= 1 and args.warmup >= 0

    import torch
    import wcg
    from wcg import mr
    from wcg.corpus import Generator, CONFIGS

    cfg = CONFIGS[CONFIG]
    nbytes, R = args.mib << 20, args.nreduce
    data = Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"]).bytes(nbytes)
    data = data[:data.rindex(b"\n") + 1] if b"\n" in data else data
    with wcg.Engine(device=0, max_input_bytes=0, max_keys=1 << 20) as src:
        parts = src.map_json(data, R)
        src.reset()
        src.map_host(data)
        nkeys, _ = src.reduce()
        merged = src.result()
        res = src.partitions(R)
    lines = sum(p.count(b"\n") for p in parts)
    log(f"{len(data)} bytes of {CONFIG}: {sum(map(len, parts))} bytes of intermediates in {R} files, "
        f"{lines} lines; {nkeys} keys, {sum(map(len, res))} bytes of -res files")

    def resident(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    d_parts = [resident(p) for p in parts]
    d_res = [resident(p) for p in res]
    keys = [mr._json_keys(p) for p in parts]
    d_keys = [resident(k) for k in keys]
    torch.cuda.synchronize()
    json_bytes, key_bytes = sum(map(len, parts)), sum(map(len, keys))
    assert key_bytes == json_bytes - 22 * lines
    del keys

    wd = tempfile.mkdtemp(prefix="import_json_bench.")
    for r in range(R):
        with open(os.path.join(wd, mr.merge_name("f", r)), "wb") as f:
            f.write(res[r])

    eng = wcg.Engine(device=0, max_input_bytes=0, max_keys=1 << 20)
    ok = True

    def answer():
        eng.reduce()
        return eng.result() == merged

    def imports(tensors, sizes, mode, stop=None):
        if stop is None:
            os.environ.pop("WCG_IMPORT_JSON_STOP", None)
        else:
            os.environ["WCG_IMPORT_JSON_STOP"] = str(stop)
        try:
            return sum(eng.import_json_device(t.data_ptr(), n, mode) for t, n in zip(tensors, sizes))
        finally:
            os.environ.pop("WCG_IMPORT_JSON_STOP", None)

    def map_keys():
        for t in d_keys:
            eng.map_device(t.data_ptr(), t.numel())
        eng.sync()

    def parent():
        for p in parts:
            k = mr._json_keys(p)
            if k:
                eng.map_host(k)
        eng.sync()

    def quiet(f):
        with contextlib.redirect_stdout(io.StringIO()):
            return f()

    ms = {k: [] for k in ("map_import_json_device", "map_check_passes", "map_check_and_write_passes", "map_write_pass",
                          "map_device_of_key_text", "res_import_json_device", "res_merge_gpu_from_files",
                          "res_host_merge_from_files")}
    host_ms = []
    psz, rsz = [len(p) for p in parts], [len(p) for p in res]
    for rep in range(args.warmup + args.reps):
        eng.reset()
        a, n1 = clock(lambda: imports(d_parts, psz, wcg.JSON_MAP))
        ok &= n1 == lines and answer()
        eng.reset()
        b, n2 = clock(lambda: imports(d_parts, psz, wcg.JSON_MAP, 1))
        c, n3 = clock(lambda: imports(d_parts, psz, wcg.JSON_MAP, 2))
        ok &= n2 == lines and n3 == lines and eng.reduce()[0] == 0       # nothing was aggregated
        eng.reset()
        d, _ = clock(map_keys)
        ok &= answer()
        eng.reset()
        e, n4 = clock(lambda: imports(d_res, rsz, wcg.JSON_RES))
        ok &= n4 == nkeys and answer()
        f, out = clock(lambda: quiet(lambda: mr.merge_gpu(eng, wd, "f", R)))
        ok &= out == merged
        g, out = clock(lambda: quiet(lambda: mr.merge(wd, "f", R)))
        ok &= out == merged
        if rep < args.warmup + args.host_reps:
            eng.reset()
            h, _ = clock(parent)
            ok &= answer()
            if rep >= args.warmup:
                host_ms.append(h)
        if rep >= args.warmup:
            for k, v in zip(ms, (a, b, c, c - b, d, e, f, g)):
                ms[k].append(v)
    eng.close()
    for r in range(R):
        os.remove(os.path.join(wd, mr.merge_name("f", r)))
    os.remove(os.path.join(wd, "mrtmp.f"))
    os.rmdir(wd)

    moved = 3 * json_bytes + 2 * key_bytes
    out = {
        "workload": CONFIG, "input_bytes": len(data), "nreduce": R, "json_bytes": json_bytes, "lines": lines,
        "key_text_bytes": key_bytes, "keys": nkeys, "res_bytes": sum(rsz),
        "reps": args.reps, "host_reps": len(host_ms), "warmup": args.warmup,
        "how": "one process; host clock around each group of calls, every call ends in a stream synchronise; the "
               "groups of one repetition run in turn; map_write_pass is check_and_write minus check, per repetition",
        "map_bytes_moved": moved, "map_floor_ms_at_8TBps": round(moved / HBM_BYTES_PER_S * 1e3, 4),
        "verified": bool(ok),
    }
    out.update({k: spread(v) for k, v in ms.items()})
    out["map_parent_json_keys_plus_map_host"] = spread(host_ms)
    log(", ".join(f"{k} {v['median_ms']:.3f} ({v['min_ms']:.3f} - {v['max_ms']:.3f})" for k, v in out.items()
                  if isinstance(v, dict)) + f" ms; floor {out['map_floor_ms_at_8TBps']} ms; verified {ok}")
    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
