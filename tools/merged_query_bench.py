#!/usr/bin/env python3
"""Querying a merged file that already exists: wcg_load_merged_device and the queries after it,
against what a caller had without them - copy the file to the host and search it there.

One merged file: that of 1 GiB of a BASELINE corpus (device-resident, map_device + reduce), copied
into a device buffer of its own; the engine that made it is closed.  A second engine then, in one
process and in turn per repetition:

  wcg_merge_runs of the file as one run, then wcg_index_merged: the two parts of a load, timed
  apart (the index is the new device pass: csrc/wcg_index.h);
  the same pair with WCG_INDEX_STAGE=0: every tile's text read in place instead of through LDS
  (the other thread layout of k_ix_write);
  wcg_load_merged_device whole (its merge part sorts no tie groups: the file is checked, not trusted);
  Engine.top(10) (a search: another n is asked in between, the cache holds one) and Engine.lookup
  of 1000 words, half of them keys of the file;
  the host path: Engine.result() (the copy), wcg.top_of_merged(file, 10), wcg.lookup_in_merged.

A host clock around each call (every one ends in a stream synchronise); medians, minimum, maximum
and quartiles.  The index time stands next to the bytes it must move (the line records read, the
query records written, the text once) over 8 TB/s.  Every answer is compared with the host's; a
mismatch exits 3.

  python tools/merged_query_bench.py --config c2|c4 [--reps 10] [--warmup 2] [--out profiles/merged_query_c2.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mit-6.824-2015_amd"))
sys.path.insert(0, ROOT)

JOBS = {
    # name: (wcg.corpus.CONFIGS key, max_keys)
    "c2": ("c2_ascii_zipf_1gib", 1 << 20),
    "c4": ("c4_utf8_zipf_64gib", 50_000_000),
}
NBYTES = 1 << 30
HBM_BYTES_PER_S = 8e12
RECORD = 32


def log(*a):
    print(f"[merged_query_bench {time.strftime('%H:%M:%S')}]", *a, flush=True)


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 2 else [ms[0]] * 3
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "n": len(ms)}


def clock(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(JOBS), default="c2")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 2 and args.warmup >= 0

    import numpy as np
    import torch
    import wcg
    from wcg.corpus import Generator, CONFIGS

    name, max_keys = JOBS[args.config]
    cfg = CONFIGS[name]
    log(f"building the {cfg['vocab']:.0e}-word generator of {name}")
    gen = Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"])
    host = np.empty(NBYTES, dtype=np.uint8)
    gen.fill_ptr(host.ctypes.data, NBYTES, first_block=0, threads=16)
    dev = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
    dev.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    del host
    with wcg.Engine(device=0, max_input_bytes=0, max_keys=max_keys) as src:
        src.reset()
        src.map_device(dev.data_ptr(), NBYTES)
        nkeys, nbytes = src.reduce()
        del dev
        mfile = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        src.result_copy_device(mfile.data_ptr())
        src.sync()
        want_top = src.top(10)
    torch.cuda.synchronize()
    log(f"the merged file: {nkeys} lines, {nbytes} bytes, resident")

    eng = wcg.Engine(device=0, max_input_bytes=0, max_keys=max(1 << 16, nkeys))
    ptr = mfile.data_ptr()
    move = 2 * RECORD * nkeys + nbytes
    res = {
        "workload": name, "input_bytes": NBYTES, "lines": nkeys, "merged_file_bytes": nbytes,
        "reps": args.reps, "warmup": args.warmup,
        "how": "one process; host clock around each call, every call ends in a stream synchronise; the calls of "
               "one repetition run in turn",
        "index_bytes_moved": move,
        "index_floor_ms_at_8TBps": round(move / HBM_BYTES_PER_S * 1e3, 4),
        "verified": True,
    }

    ms = {k: [] for k in ("merge_runs_one_run", "index_merged", "merge_runs_one_run_again", "index_merged_in_place",
                          "load_merged_device", "top10_after_load", "lookup1000_after_load",
                          "host_result_copy", "host_top_of_merged_10", "host_lookup_in_merged_1000")}
    merged = b""
    words = []
    for rep in range(args.warmup + args.reps):
        os.environ.pop("WCG_INDEX_STAGE", None)
        a, _ = clock(lambda: eng.merge_runs(ptr, [nbytes]))
        b, nl = clock(eng.index_merged)
        os.environ["WCG_INDEX_STAGE"] = "0"
        a2, _ = clock(lambda: eng.merge_runs(ptr, [nbytes]))
        b2, nl2 = clock(eng.index_merged)
        os.environ.pop("WCG_INDEX_STAGE", None)
        c, nl3 = clock(lambda: eng.load_merged_device(ptr, nbytes))
        eng.top(7)                                           # the cache holds one n
        d, top = clock(lambda: eng.top(10))
        if not words:
            merged = eng.result()
            keys = [l.rpartition(b": ")[0] for l in merged.split(b"\n") if l]
            rnd = random.Random(21)
            words = [keys[rnd.randrange(nkeys)] for _ in range(500)] + [keys[rnd.randrange(nkeys)] + b"zq" for _ in range(500)]
            rnd.shuffle(words)
            del keys
        e, got = clock(lambda: eng.lookup(words))
        f, merged = clock(eng.result)
        g, htop = clock(lambda: wcg.top_of_merged(merged, 10))
        h, hgot = clock(lambda: wcg.lookup_in_merged(merged, words))
        if not (nl == nl2 == nl3 == nkeys and top == htop == want_top and got == hgot and len(merged) == nbytes):
            res["verified"] = False
        if rep >= args.warmup:
            for k, v in zip(ms, (a, b, a2, b2, c, d, e, f, g, h)):
                ms[k].append(v)
    eng.close()
    res.update({k: spread(v) for k, v in ms.items()})
    res["index_over_floor"] = round(res["index_merged"]["median_ms"] / res["index_floor_ms_at_8TBps"], 1)
    res["host_copy_plus_top_median_ms"] = round(res["host_result_copy"]["median_ms"] + res["host_top_of_merged_10"]["median_ms"], 3)
    res["host_copy_plus_lookup_median_ms"] = round(res["host_result_copy"]["median_ms"] + res["host_lookup_in_merged_1000"]["median_ms"], 3)
    log(f"merge {res['merge_runs_one_run']['median_ms']:.3f} ms, index {res['index_merged']['median_ms']:.3f} ms "
        f"(in place {res['index_merged_in_place']['median_ms']:.3f} ms, floor {res['index_floor_ms_at_8TBps']:.4f} ms), "
        f"load {res['load_merged_device']['median_ms']:.3f} ms, top(10) {res['top10_after_load']['median_ms']:.3f} ms, "
        f"lookup(1000) {res['lookup1000_after_load']['median_ms']:.3f} ms; host copy + top "
        f"{res['host_copy_plus_top_median_ms']:.1f} ms, copy + lookup {res['host_copy_plus_lookup_median_ms']:.1f} ms; "
        f"verified {res['verified']}")

    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)
    if not res["verified"]:
        sys.exit(3)


if __name__ == "__main__":
    main()
