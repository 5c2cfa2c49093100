#!/usr/bin/env python3
"""wcg_lookup and wcg_range against what a caller had to do before them: copy the merged file to
the host and look the words up there.

One job (1 GiB of a BASELINE corpus, device-resident, map_device + reduce).  The baseline is
Engine.result() (the copy), one parse of the file into a dict and a sorted key list (timed once:
an index a caller builds per job), then dict lookups, or a bisect of the key list and a slice of
the file for a prefix.  Against it, in one process and in turn per repetition:

  Engine.lookup of 1, 10^3 and 10^6 words, half of them keys of the job (sampled), half not;
  wcg_lookup itself on prebuilt arrays (Engine.lookup minus Python's list handling);
  wcg_lookup_device on queries already in device memory, then a stream synchronise (the kernel);
  Engine.prefix(p), p chosen among the job's own keys to select about 0.1 % of them; a prefix q
  selecting about as many is asked in between, so that every timed call searches, sizes, formats
  and copies (the cache holds one range); then the same p again (the cached lines: a copy).

A host clock around each call (every one ends in a stream synchronise); medians, minimum, maximum
and the quartiles.  Every timed result is compared with the baseline's answer; a mismatch exits 3.

  python tools/lookup_bench.py --config c2|c4 [--reps 20] [--warmup 3] [--out profiles/lookup_bench_c2.json]
"""
from __future__ import annotations

import argparse
import bisect
import ctypes
import itertools
import json
import math
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
BATCHES = (1, 1000, 1_000_000)


def log(*a):
    print(f"[lookup_bench {time.strftime('%H:%M:%S')}]", *a, flush=True)


def spread(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 2 else [ms[0]] * 3
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "n": len(ms)}


def clock(f):
    t = time.perf_counter()
    out = f()
    return (time.perf_counter() - t) * 1e3, out


def pick_prefixes(keys, target):
    """two prefixes of the job's own keys that select about `target` keys each (bisect on the sorted list)"""
    import wcg
    found = {}
    for pos in range(1, 40):
        k = keys[len(keys) * pos // 40]
        for L in range(1, len(k) + 1):
            p = k[:L]
            s = wcg.prefix_succ(p)
            n = (bisect.bisect_left(keys, s) if s is not None else len(keys)) - bisect.bisect_left(keys, p)
            found[p] = n
    ranked = sorted(found, key=lambda p: (abs(math.log(max(found[p], 0.5) / target)), p))
    first = ranked[0]
    second = next(p for p in ranked[1:] if not p.startswith(first) and not first.startswith(p))   # other lines
    return [(first, found[first]), (second, found[second])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(JOBS), default="c2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    log("1 GiB generated and resident")

    eng = wcg.Engine(device=0, max_input_bytes=0, max_keys=max_keys)
    lib = eng._lib
    for _ in range(2):                                   # the second job runs on sized buffers
        eng.reset()
        eng.map_device(dev.data_ptr(), NBYTES)
        nkeys, nbytes = eng.reduce()
    nrec = max(nkeys, eng.stats()["emitted"])            # sorted records (merged duplicates included)
    del dev
    log(f"{nkeys} keys, {nrec} sorted records, merged file {nbytes} bytes")

    # ---- the baseline: the copy, and the index a caller builds from it once per job
    copy_ms = []
    merged = b""
    for _ in range(max(3, min(args.reps, 10))):
        dt, merged = clock(eng.result)
        copy_ms.append(dt)
    t = time.perf_counter()
    keys, ends, table, end = [], [], {}, 0
    for line in merged.split(b"\n"):
        if line:
            k, _, c = line.rpartition(b": ")
            end += len(line) + 1
            keys.append(k)
            ends.append(end)
            table[k] = int(c)
    parse_ms = (time.perf_counter() - t) * 1e3
    assert len(keys) == nkeys and end == nbytes
    log(f"copy {statistics.median(copy_ms):.3f} ms, parse into dict + key list {parse_ms:.0f} ms")

    rnd = random.Random(20)
    res = {
        "workload": name, "input_bytes": NBYTES, "nkeys": nkeys, "nrec": nrec, "merged_file_bytes": nbytes,
        "search_steps": math.ceil(math.log2(nrec + 1)),
        "reps": args.reps, "warmup": args.warmup,
        "how": "one process; host clock around each call, every call ends in a stream synchronise; the "
               "calls of one repetition run in turn; each batch is half keys of the job, half absent words",
        "baseline_result_copy": spread(copy_ms),
        "baseline_parse_once_ms": round(parse_ms, 1),
        "lookup": {}, "verified": True,
    }

    # ---- point queries
    for nq in BATCHES:
        half = (nq + 1) // 2
        words = [keys[rnd.randrange(nkeys)] for _ in range(half)] + \
                [keys[rnd.randrange(nkeys)] + b"zq" for _ in range(nq - half)]
        rnd.shuffle(words)
        blob = b"".join(words)
        off = (ctypes.c_uint64 * (nq + 1))(0, *itertools.accumulate(map(len, words)))
        counts = (ctypes.c_uint64 * nq)()
        d_keys = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda")
        d_off = torch.tensor(list(off), dtype=torch.int64, device="cuda")
        d_cnt = torch.zeros(nq, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def host_dict():
            return [table.get(w, 0) for w in words]

        def c_call():
            assert lib.wcg_lookup(eng._ctx, blob, off, nq, counts) == 0

        def device_call():
            eng.lookup_device(d_keys.data_ptr(), d_off.data_ptr(), nq, d_cnt.data_ptr())
            eng.sync()

        ms = {"engine_lookup": [], "wcg_lookup": [], "wcg_lookup_device_and_sync": [], "host_dict_lookups": []}
        want = host_dict()
        for rep in range(args.warmup + args.reps):
            a, got = clock(lambda: eng.lookup(words))
            b, _ = clock(c_call)
            c, _ = clock(device_call)
            d, _ = clock(host_dict)
            ok = got == want and list(counts) == want and \
                [x & (2 ** 64 - 1) for x in d_cnt.cpu().tolist()] == want
            if not ok:
                res["verified"] = False
            if rep >= args.warmup:
                ms["engine_lookup"].append(a); ms["wcg_lookup"].append(b)
                ms["wcg_lookup_device_and_sync"].append(c); ms["host_dict_lookups"].append(d)
        r = {k: spread(v) for k, v in ms.items()}
        r["present"] = sum(1 for x in want if x)
        r["baseline_copy_plus_dict_median_ms"] = round(res["baseline_result_copy"]["median_ms"] +
                                                       r["host_dict_lookups"]["median_ms"], 4)
        r["baseline_copy_plus_dict_min_ms"] = round(res["baseline_result_copy"]["min_ms"] +
                                                    r["host_dict_lookups"]["min_ms"], 4)
        r["engine_lookup_below_baseline_ranges_apart"] = r["engine_lookup"]["max_ms"] < r["baseline_copy_plus_dict_min_ms"]
        t_dev = r["wcg_lookup_device_and_sync"]["median_ms"] * 1e-3
        r["device_searches_per_s"] = round(nq / t_dev)
        r["device_record_loads_per_s"] = round(nq * res["search_steps"] / t_dev)
        res["lookup"][str(nq)] = r
        log(f"nq {nq}: Engine.lookup {r['engine_lookup']['median_ms']:.3f} ms, wcg_lookup "
            f"{r['wcg_lookup']['median_ms']:.3f} ms, device {r['wcg_lookup_device_and_sync']['median_ms']:.3f} ms, "
            f"copy + dict {r['baseline_copy_plus_dict_median_ms']:.3f} ms, verified {res['verified']}")
        del d_keys, d_off, d_cnt

    # ---- a prefix selecting about 0.1 % of the keys
    (p, np_), (q, nq_) = pick_prefixes(keys, max(1.0, nkeys / 1000))

    def host_prefix(pp):
        s = wcg.prefix_succ(pp)
        i = bisect.bisect_left(keys, pp)
        j = bisect.bisect_left(keys, s) if s is not None else len(keys)
        return merged[ends[i - 1] if i else 0: ends[j - 1] if j else 0]

    ms = {"engine_prefix": [], "engine_prefix_cached": [], "host_bisect_and_slice": []}
    want_p, want_q = host_prefix(p), host_prefix(q)
    assert want_p.count(b"\n") == np_ and want_p == wcg.range_of_merged(want_p, p, wcg.prefix_succ(p))
    for rep in range(args.warmup + args.reps):
        a, got = clock(lambda: eng.prefix(p))
        b, again = clock(lambda: eng.prefix(p))
        other = eng.prefix(q)                              # the cache holds one range
        c, _ = clock(lambda: host_prefix(p))
        if not (got == want_p and again == want_p and other == want_q):
            res["verified"] = False
        if rep >= args.warmup:
            ms["engine_prefix"].append(a); ms["engine_prefix_cached"].append(b); ms["host_bisect_and_slice"].append(c)
    r = {k: spread(v) for k, v in ms.items()}
    r.update({"prefix": p.decode(errors="replace"), "lines": np_, "bytes": len(want_p),
              "share_of_keys": round(np_ / nkeys, 6), "other_prefix_lines": nq_})
    r["baseline_copy_plus_bisect_median_ms"] = round(res["baseline_result_copy"]["median_ms"] +
                                                     r["host_bisect_and_slice"]["median_ms"], 4)
    r["baseline_copy_plus_bisect_min_ms"] = round(res["baseline_result_copy"]["min_ms"] +
                                                  r["host_bisect_and_slice"]["min_ms"], 4)
    r["engine_prefix_below_baseline_ranges_apart"] = r["engine_prefix"]["max_ms"] < r["baseline_copy_plus_bisect_min_ms"]
    res["prefix"] = r
    log(f"prefix {p!r}: {np_} lines, Engine.prefix {r['engine_prefix']['median_ms']:.3f} ms "
        f"(cached {r['engine_prefix_cached']['median_ms']:.3f} ms), copy + bisect "
        f"{r['baseline_copy_plus_bisect_median_ms']:.3f} ms, verified {res['verified']}")
    eng.close()

    if args.out and args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)
    if not res["verified"]:
        sys.exit(3)


if __name__ == "__main__":
    main()
