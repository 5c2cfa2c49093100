"""Config 5 with one OS process per worker (worker.go:60-92, master.go:29-88).

The master (wcg/mr.py MapReduce) runs in the test process; every worker is its own process
started with subprocess.Popen - on the GPU box `python -m wcg.wc worker <master> <me>`, which
binds one GPU (HIP_VISIBLE_DEVICES / WCG_DEVICE per process; the box has one, so they share it).
Failures injected:
  * a worker with an RPC budget of 10 (worker.go:80-89: it stops accepting after 10);
  * a worker SIGKILLed while it runs a DoJob (its "Dojob ..." line has appeared on stdout), so
    the master's call fails and the job is re-executed on another worker; job outputs are written
    temp-then-rename, so the killed worker leaves no truncated file under a reference name.
Checked: the merged file and all nReduce -res-<r> files against the oracle, and CleanupFiles
finds exactly the reference's file names.  Input: a slice of the C2 corpus, nMap >= 32, R = 64.
"""
import os
import signal
import subprocess
import sys
import threading
import time

import pytest

from tests.oracle_bridge import wc_ref
from tests.test_mr_workers import sock  # noqa: F401  (fixture: a short directory for the sockets)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mit-6.824-2015_amd")


def _expected(data):
    return wc_ref.word_count(b"".join(wc_ref.split(data, 1)))


class Proc:
    def __init__(self, argv, env, cwd):
        self.p = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=cwd)
        self.lines = []
        self.dojob = threading.Event()
        threading.Thread(target=self._read, daemon=True).start()

    def _read(self):
        for line in self.p.stdout:
            self.lines.append(line)
            if line.startswith(b"Dojob"):
                self.dojob.set()


def _run(tmp_path, sock, worker_argv, nmap=32, nreduce=64, nbytes=24 << 20, kill_one=True, timeout=300):
    from wcg import mr
    from wcg.corpus import Generator, CONFIGS
    cfg = CONFIGS["c2_ascii_zipf_1gib"]
    data = Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"]).bytes(nbytes)
    path = tmp_path / "824-mrinput.txt"
    path.write_bytes(data)
    master = str(sock / "mr-master")
    job = mr.MapReduce(nmap, nreduce, str(path), master, str(tmp_path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]), PYTHONUNBUFFERED="1")
    procs = []
    try:
        def start(name, nrpc):
            # the worker's working directory is the shared "file system" (wc.go workers use cwd)
            procs.append(Proc(worker_argv(master, str(sock / name), nrpc), dict(env, WCG_NRPC=str(nrpc)),
                              str(tmp_path)))
            return procs[-1]
        victim = start("w-victim", -1) if kill_one else None
        start("w-budget10", 10)
        start("w-a", -1)
        start("w-b", -1)
        if victim is not None:
            assert victim.dojob.wait(120), b"".join(victim.lines)[-2000:]
            time.sleep(0.05)                                    # inside its DoJob
            victim.p.send_signal(signal.SIGKILL)
        merged = job.wait(timeout)
    finally:
        for pr in procs:
            if pr.p.poll() is None:
                pr.p.kill()
            pr.p.wait(30)
    counts = _expected(data)
    assert merged == wc_ref.merged_output(counts)
    for r in range(nreduce):
        assert (tmp_path / mr.merge_name(job.file, r)).read_bytes() == wc_ref.res_file(counts, nreduce, r), r
    job.cleanup_files()
    left = [f for f in os.listdir(tmp_path) if f.startswith("mrtmp.")]
    assert left == [], left
    out = b"".join(b"".join(pr.lines) for pr in procs)
    assert b"Dojob" in out and b"DoMap: read split" in out and b"DoReduce: read" in out
    if kill_one:
        assert procs[0].p.returncode == -signal.SIGKILL
    return job


def _standin_argv(tmp):
    return lambda master, me, nrpc: [sys.executable, os.path.join(ROOT, "tests", "standin_worker.py"), master, me,
                                     str(nrpc), str(tmp)]


def test_worker_processes_sigkill_cpu_standin(tmp_path, sock):
    _run(tmp_path, sock, _standin_argv(tmp_path), nbytes=3 << 20)


@pytest.mark.gpu
def test_worker_processes_sigkill_gpu(tmp_path, sock, built):
    # wc.go's worker CLI (nRPC = 100; the budget knob WCG_NRPC is set per process by _run)
    _run(tmp_path, sock, lambda master, me, nrpc: [sys.executable, "-m", "wcg.wc", "worker", master, me])
