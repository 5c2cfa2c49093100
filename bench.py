#!/usr/bin/env python3
"""Word-count throughput on MI355X: input GB/s (whole node) and fraction of the HBM roofline.

A step = one word-count job over device-resident synthetic input: reset tables -> map kernels
(tokenize + aggregate) -> sort + format the merged "key: count\\n" output in HBM.
  N = 1: BASELINE config 2 (1 GiB ASCII Zipf, V=1e5, s=1.0, seed 42), the metric's config.
  N > 1: BASELINE config 3 (16 GiB of the same generator, seed 43, nReduce 64) split over the
         N ranks (strong scaling): map -> export by owner (ihash % 64) % N -> RCCL all-to-all-v ->
         owners import, sort and format their partitions -> rank 0 merges the owners' sorted runs.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, runs W warm-up and K timed steps of the loop its value is made of, writes the
last job's merged file with --dump-outputs, and prints one JSON line.  --full adds everything else:
after the timed steps the merged file is checked byte for byte against the C oracle (N > 1:
against the sum of every rank's oracle counts; a mismatch exits 3 without printing a rate), N = 1
also times the one-engine loops, and the line carries per-phase times, the end-to-end file job
and the CPU baselines.
N > 1: one rank per GPU (backend nccl = RCCL).  Started by an external torch.distributed.run, or,
when WORLD_SIZE is not set, by this script itself (wcg/launch.py) before any GPU call.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "mit-6.824-2015_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # k_map's launch time falls over its first ~10 launches on a fresh process (978 -> 890 us in
    # profiles/r03_kernel_trace_v8: clocks and page tables warming up), so the default warm-up
    # covers that; a step is ~1.3 ms, the whole default run is dominated by corpus generation
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--workload", default=None,
                    help="default: c2_ascii_zipf_1gib at N = 1 (BASELINE config 2, the metric's config); "
                         "c3_ascii_zipf_16gib at N > 1 (BASELINE config 3: 16 GiB strong-scaled over N, nReduce 64)")
    ap.add_argument("--bytes", type=int, default=None, help="total input bytes (default: the workload's size)")
    ap.add_argument("--nreduce", type=int, default=64)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline loop: the check of the result against the oracle, the other "
                         "step loops (N = 1), the instrumented phase steps, the end-to-end file job and the "
                         "CPU baselines (the --no-* switches below leave single legs out)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed job left (the merged file) "
                         "as DIR/<name>.npy")
    ap.add_argument("--cpu-sample-mib", type=int, default=256)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--sync-steps", action="store_true",
                    help="N = 1: every timed step waits for its reduce (wcg_reduce) instead of queuing the "
                         "next job behind it (wcg_reduce_async)")
    ap.add_argument("--contexts", type=int, default=2,
                    help="N = 1: engines (each on its own stream) the multi-context loop deals its jobs to; "
                         "1 skips that loop (at most 4: one hardware queue each)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo: rehearsal of the N > 1 path with host-staged records, ranks may share a GPU")
    # below the driver's 600 s bench limit, so that the launcher's own bounded stop (and every
    # rank's stack dump on SIGTERM) happens before an outside kill
    ap.add_argument("--launch-timeout", type=float, default=480.0,
                    help="--gpus N > 1 without an external launcher: seconds before the rank processes are stopped")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "traffic_latest.json"),
                    help="PMC-derived HBM bytes per map launch (written by tools/pmc_traffic.py)")
    return ap.parse_args()


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(directory, merged):
    """--dump-outputs: what a caller of the timed path receives from its last job, the merged
    "key: count\\n" file (wcg_result_copy), as merged.npy (one float32 per byte; of a file too large
    for the 64 MB cap, the bytes at a fixed seeded set of offsets), and merged_size.npy (float64:
    the file's bytes and lines, a line per key)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    b = np.frombuffer(merged, dtype=np.uint8)
    cap = (DUMP_CAP_BYTES - 4096) // 4
    if b.size > cap:
        b = b[np.unique(np.random.default_rng(0).integers(0, b.size, cap))]
    np.save(os.path.join(directory, "merged.npy"), b.astype(np.float32))
    np.save(os.path.join(directory, "merged_size.npy"),
            np.array([len(merged), merged.count(b"\n")], dtype=np.float64))


def _timed_file_port(fn, data, fname):
    from tests import oracle_bridge as ob
    d = tempfile.mkdtemp(prefix="wcg-cpu-", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        with open(os.path.join(d, fname), "wb") as f:
            f.write(data)
        t0 = time.perf_counter()
        rc = fn(d)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError("cpu baseline failed")
        ok = open(os.path.join(d, "mrtmp." + fname), "rb").read() == ob.merged(data)
    finally:
        for f in os.listdir(d):
            os.unlink(os.path.join(d, f))
        os.rmdir(d)
    return dt, ok


def cpu_baselines(cfg, sample_bytes):
    """CPU baselines on this host's cores, on the first `sample_bytes` of the same corpus (the
    reference's Go code cannot run here: no Go toolchain; these are the oracle's ports):
      cpu_baseline           RunSingle(nMap=5, nReduce=3) file-based port (oracle/mr_port.c: Split,
                             DoMap with one JSON write(2) per token, DoReduce, Merge), 1 thread;
      cpu_baseline_parallel  the master/worker path's work, W worker threads taking map then
                             reduce jobs (mrp_run_parallel, nMap = 4W, nReduce = 64);
      cpu_restatement_all_cores  the in-memory word count (oracle/wc_oracle.c) on all cores."""
    from tests import oracle_bridge as ob
    from wcg.corpus import Generator
    data = Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"]).bytes(sample_bytes)
    fname = "cpu-sample.txt"
    nproc = os.cpu_count() or 1
    W = max(1, min(16, nproc))       # the box grants one GPU's share of its host: 16 threads
    dt1, ok1 = _timed_file_port(lambda d: ob.run_single_files(d, fname, 5, 3), data, fname)
    dtw, okw = _timed_file_port(lambda d: ob.run_parallel_files(d, fname, 4 * W, 64, W), data, fname)
    t0 = time.perf_counter()
    ob.Result(data, W)
    dtm = time.perf_counter() - t0
    mib = sample_bytes >> 20
    return (
        {"value": round(sample_bytes / dt1 / 1e9, 6), "unit": "GB/s", "cores": 1, "kind": "port",
         "host_nproc": nproc,
         "sample": f"first {mib} MiB of the same corpus, RunSingle(nMap=5, nReduce=3) file-based port "
                   f"incl. split/intermediate/res files on tmpfs ({dt1:.1f} s)", "merged_equal_gpu_oracle": ok1},
        {"value": round(sample_bytes / dtw / 1e9, 6), "unit": "GB/s", "cores": W, "kind": "port",
         "host_nproc": nproc, "thread_cap": 16,
         "sample": f"first {mib} MiB, master/worker path: {W} worker threads, nMap={4 * W}, nReduce=64, "
                   f"files on tmpfs ({dtw:.1f} s)", "merged_equal_gpu_oracle": okw},
        {"value": round(sample_bytes / dtm / 1e9, 6), "unit": "GB/s", "cores": W, "kind": "port",
         "host_nproc": nproc, "thread_cap": 16,
         "sample": f"first {mib} MiB, in-memory word count (oracle/wc_oracle.c) on {W} threads ({dtm:.1f} s)"},
    )


def ingest_ceilings(path, n, reps=3):
    """The two legs wcg_map_file overlaps, each measured alone on this box: the host read of the
    file (16 threads of pread into a pinned buffer, as the ingest's reader pool does) and the
    pinned host -> HBM copy (PCIe).  The pipeline cannot beat the slower of the two."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    host = torch.empty(n, dtype=torch.uint8).pin_memory()
    mv = memoryview(host.numpy()).cast("B")
    T = 16
    fd = os.open(path, os.O_RDONLY)
    try:
        def rd(t):
            a, b = n * t // T, n * (t + 1) // T
            while a < b:
                r = os.preadv(fd, [mv[a:b]], a)
                if r <= 0:
                    raise OSError("short read")
                a += r
        best_r = None
        with ThreadPoolExecutor(T) as ex:
            for _ in range(reps):
                t0 = time.perf_counter()
                list(ex.map(rd, range(T)))
                dt = time.perf_counter() - t0
                best_r = dt if best_r is None else min(best_r, dt)
    finally:
        os.close(fd)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    best_c = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev.copy_(host, non_blocking=True)
        e1.record()
        e1.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        best_c = dt if best_c is None else min(best_c, dt)
    # both legs at once (what the ingest does): the reader threads and the copy engine share the
    # host's memory bandwidth (a pread moves each byte twice through host DRAM, the DMA once)
    host2 = torch.empty(n, dtype=torch.uint8).pin_memory()
    mv2 = memoryview(host2.numpy()).cast("B")
    fd = os.open(path, os.O_RDONLY)
    try:
        def rd2(t):
            a, b = n * t // T, n * (t + 1) // T
            while a < b:
                r = os.preadv(fd, [mv2[a:b]], a)
                if r <= 0:
                    raise OSError("short read")
                a += r
        with ThreadPoolExecutor(T) as ex:
            t0 = time.perf_counter()
            dev.copy_(host, non_blocking=True)
            list(ex.map(rd2, range(T)))
            torch.cuda.synchronize()
            both = time.perf_counter() - t0
    finally:
        os.close(fd)
    del dev, host, host2
    r, c = n / best_r / 1e9, n / best_c / 1e9
    return {"host_read_gbs": round(r, 2), "h2d_pinned_gbs": round(c, 2), "bound_gbs": round(min(r, c), 2),
            "concurrent_gbs": round(n / both / 1e9, 2),
            "how": "each leg alone: 16-thread pread of the tmpfs file into pinned memory; pinned H2D copy "
                   "(torch events); the ingest overlaps them, so the slower one bounds end_to_end.  "
                   "concurrent_gbs: the same n bytes read AND copied at once (both legs together), "
                   "host-DRAM-bound on boxes where the two legs share its bandwidth"}


def end_to_end(keys_cap, cfg, n, reps=5):
    """Split -> merged file on one GPU from an input file: wcg_map_file (the pinned
    double-buffered ingest: host reads || PCIe copy || map kernels) + reduce + D2H + write of
    mrtmp.<f>.  The file sits in tmpfs (page cache), so this is the host-read + PCIe-bound rate,
    reported beside the device-resident metric, never as it.  An engine of its own, on the
    engine's own stream (r04: the bench's engine, bound to a torch stream, measured 30.4 GB/s on a
    box where a fresh engine's ingest took 25-26 ms per GiB, profiles/r04_ingest_*); the best of
    `reps` jobs, the first of which also allocates the staging buffers."""
    import wcg
    from wcg.corpus import Generator
    d = tempfile.mkdtemp(prefix="wcg-e2e-", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(d, "input.txt")
    try:
        import torch
        host = torch.empty(n, dtype=torch.uint8)
        Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"]).fill_ptr(host.data_ptr(), n)
        host.numpy().tofile(path)
        del host
        best, best_parts = None, None
        with wcg.Engine(device=torch.cuda.current_device(), max_input_bytes=0, max_keys=keys_cap) as eng:
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.reset()
                mapped, size = eng.map_file(path)
                t1 = time.perf_counter()
                eng.reduce()
                out = eng.result()
                with open(os.path.join(d, "mrtmp.input.txt"), "wb") as f:
                    f.write(out)
                dt = time.perf_counter() - t0
                # the job's own breakdown, read after the job (reading it waits for the streams)
                ing = eng.ingest_stats()
                parts = {"reader_ms": ing["read_ms"], "slot_wait_ms": ing["slot_wait_ms"],
                         "copy_ms": ing["copy_ms"], "copy_engine_idle_frac": ing["copy_engine_idle_frac"],
                         "map_kernels_ms": ing["map_ms"], "ingest_host_ms": ing["host_issue_ms"],
                         "ingest_device_span_ms": ing["device_span_ms"],
                         "reduce_and_write_ms": (t0 + dt - t1) * 1e3, "chunks": int(ing["chunks"])}
                if best is None or dt < best:
                    best, best_parts = dt, {k: round(v, 3) if isinstance(v, float) else v for k, v in parts.items()}
        ceil = ingest_ceilings(path, n)
        v = n / best / 1e9
        return {"value": round(v, 3), "unit": "GB/s", "seconds": round(best, 4),
                "path": "input file in tmpfs -> wcg_map_file (Split + DoMap) -> reduce -> mrtmp.<f> written",
                "mapped_bytes": mapped, "reps": reps, "ceilings": ceil,
                "frac_of_bound": round(v / ceil["bound_gbs"], 3),
                "breakdown": dict(best_parts, how=(
                    "the best job's own timers (wcg_ingest_stats): reader_ms = pread + line scan on the "
                    "calling thread and its reader pool, slot_wait_ms = waiting for a free pinned staging "
                    "slot (the copy behind), copy_ms = the chunks' H2D copies (events on the copy stream), "
                    "copy_engine_idle_frac = 1 - copy_ms / (first copy start .. last copy end), "
                    "map_kernels_ms = the chunks' map kernels (events on the work stream), "
                    "ingest_host_ms = wcg_map_file until its last chunk was issued, "
                    "reduce_and_write_ms = wcg_reduce + result copy + file write after wcg_map_file returned"))}
    finally:
        for f in os.listdir(d):
            os.unlink(os.path.join(d, f))
        os.rmdir(d)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # a plain `python bench.py --gpus N`: start the N rank processes here (one per GPU, under
        # torch.distributed.run) and relay rank 0's line.  This process never initialises a GPU;
        # a failed rank or a job past --launch-timeout ends the run with a non-zero status.
        from wcg.launch import launch_ranks
        sys.exit(launch_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus, args.launch_timeout))
    import torch
    import torch.distributed as dist
    import wcg
    from wcg.corpus import Generator, CONFIGS, BLOCK
    from wcg import distributed as wd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    gloo = args.dist_backend == "gloo"
    if gloo:                                  # rehearsal: ranks may share the box's GPU(s)
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    workload = args.workload or ("c2_ascii_zipf_1gib" if world == 1 else "c3_ascii_zipf_16gib")
    cfg = dict(CONFIGS[workload])
    total = args.bytes or cfg["nbytes"]
    strong = workload.startswith("c3")        # C3: 16 GiB in all, split over the N GPUs
    if strong:
        nblocks = (total + BLOCK - 1) // BLOCK
        b0, b1 = nblocks * rank // world, nblocks * (rank + 1) // world
        first_block, n = b0, min(b1 * BLOCK, total) - b0 * BLOCK
    else:                                     # weak: every rank maps its own `total` bytes
        first_block, n = rank * ((total + BLOCK - 1) // BLOCK), total
    # ---- synthetic input for this rank: generator blocks [first_block, ...), line-aligned, in HBM
    host = torch.empty(n, dtype=torch.uint8).pin_memory()
    gen = Generator(cfg["mode"], cfg["vocab"], cfg["zipf_s"], cfg["seed"])
    gen.fill_ptr(host.data_ptr(), n, first_block=first_block)
    dev = host.to(f"cuda:{local}", non_blocking=False)
    torch.cuda.synchronize()

    # one stream for the engine's kernels and the collectives (stream-ordered hand-overs, no host
    # waits between export, all-to-all and import)
    work = torch.cuda.Stream()
    # N = 1: the other engines' streams, next to the first so that HIP gives each its own hardware
    # queue (GPU_MAX_HW_QUEUES = 4 here; a second stream first used only in the multi-context loop
    # got `work`'s queue and the two engines' jobs ran one after the other: r06_experiments)
    nctx = max(1, min(args.contexts, 4)) if world == 1 else 1
    xstreams = [torch.cuda.Stream() for _ in range(nctx - 1)]
    # (the queue is dealt at a stream's first use: the streams are used here, one after another)
    for s_ in [work] + xstreams:
        with torch.cuda.stream(s_):
            torch.zeros(1, device=f"cuda:{local}")
    torch.cuda.synchronize()
    torch.cuda.set_stream(work)
    stream = work.cuda_stream
    # table capacity: twice the vocabulary, but no more keys than one per 32 input bytes (C4's densest
    # slice has one distinct key per 45 bytes).  Oversized tables cost time: k_compact scans every
    # slot, and the table probes of k_agg/k_long spread over more pages (TLB) and miss the
    # 256 MB MALL.  A table too small for the input fails loudly (WCG_EFULL), never silently.
    keys_cap = max(min(2 * cfg["vocab"], n // 32), 1 << 18)
    eng = wcg.Engine(device=local, max_input_bytes=0, max_keys=keys_cap)
    eng.set_stream(stream)
    # HIP events around the map kernel of every timed job (timing mode 3: summed by the engine, read
    # once after the timed loop; each event is a ~5 us bubble, so the other phases are timed on
    # separate instrumented steps after the timed loop, mode 2)
    eng.enable_timing(3)
    teng = wd.TorchEngine(eng, stream, host_staging=gloo)
    if world > 1 and not gloo:
        # RCCL inside libwcg: wcg_exchange (the shuffle) and wcg_gather_merge (Merge at rank 0)
        wd.init_comm(teng)

    # N > 1: each rank names the stage it enters on stderr for the first warm-up step and the first
    # timed step (a hang is then attributed to map / exchange / reduce / gather), and dumps every
    # thread's stack when the launcher stops it (SIGTERM)
    nstep = [0]
    mark_steps = {0, args.warmup}

    def stage(name):
        if world > 1 and nstep[0] in mark_steps:
            sys.stderr.write(f"bench rank {rank}/{world}: step {nstep[0]} {name}\n")
            sys.stderr.flush()

    if world > 1:
        import faulthandler
        import signal
        faulthandler.register(signal.SIGTERM, chain=True)

    def step(pipelined=False):
        """one job: this rank's map (N = 1: + DoReduce and Merge; N > 1: + shuffle, owners'
        DoReduce, Merge of the runs at rank 0).  pipelined (N = 1): the reduce is queued with its
        size read-back and not waited for (wcg_reduce_async), so the host queues the next job
        behind it and back-to-back jobs run without host gaps; each job still runs in full"""
        stage("map")
        eng.reset()
        eng.map_device(dev.data_ptr(), n)
        if world == 1:
            if pipelined:
                eng.reduce_async()
            else:
                eng.reduce()
            nstep[0] += 1
            return
        stage("exchange+reduce")
        wd.shuffle_reduce(teng, args.nreduce)            # owners: DoReduce of their partitions
        stage("gather")
        wd.gather_merge(teng, fetch=False)               # rank 0: k-way merge of the sorted runs
        stage("done")
        nstep[0] += 1

    pipe = world == 1 and not args.sync_steps
    # N = 1 (r06): jobs may also be dealt in turn to several engines (contexts), each on its own
    # stream: every job is the same full reset + map + reduce, but the next job's k_map starts on
    # the CUs that the previous job's aggregation tail and one-launch reduce leave idle (one
    # engine's jobs are strictly ordered on its stream).  An engine's previous job is waited for
    # (its status read back) before the engine is reused; every engine's last output is verified.
    two = pipe and nctx > 1
    engs, pend = [eng], [False] * nctx
    if two:
        for s_ in xstreams:
            e_ = wcg.Engine(device=local, max_input_bytes=0, max_keys=keys_cap)
            e_.set_stream(s_.cuda_stream)
            engs.append(e_)

    def step2(i):
        j = i % len(engs)
        if pend[j]:
            engs[j].reduce_wait()
        engs[j].reset()
        engs[j].map_device(dev.data_ptr(), n)
        engs[j].reduce_async()
        pend[j] = True

    def drain2():
        for j in range(len(engs)):
            if pend[j]:
                engs[j].reduce_wait()
                pend[j] = False

    # A plain run times one K-step loop, the one its value is made of: at N = 1 the multi-context
    # loop (with --contexts 1 the one-engine pipelined loop, with --sync-steps the synced one), at
    # N > 1 the ranks' loop.  --full also runs the other N = 1 loops (the fastest is then the
    # value, step_mode names it), the instrumented phase steps, the check against the oracle, the
    # end-to-end file job and the CPU baselines.
    full = args.full
    one_engine_loop = full or not two
    dt = map_sum = synced_ms = two_ms = None
    step_ms = []
    last = eng                                # the engine that ran the last timed job
    if one_engine_loop:
        for _ in range(args.warmup):
            step(pipe)
        if pipe:
            eng.reduce_wait()
        eng.enable_timing(3)                      # a new epoch: the timed steps only
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        # N > 1 (and --sync-steps): every step ends in a host wait (wcg_reduce reads back the formatted
        # size; the N > 1 Merge is synchronous at root), so the host clock between steps times each step
        t0 = time.perf_counter()
        marks = [t0]
        for _ in range(args.steps):
            step(pipe)
            marks.append(time.perf_counter())
        if pipe:
            eng.reduce_wait()                     # the last job's sizes and status (errors surface here)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if not pipe:
            step_ms = [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]
        if world > 1:
            tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if gloo else "cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        map_sum, map_launches = eng.timings()         # k_map device ms, summed over the timed steps
        assert map_launches == args.steps, (map_launches, args.steps)
    if pipe and full:
        # the same K jobs with a host wait at the end of each (wcg_reduce): the per-step spread on
        # the host clock, and the rate a caller that waits for every job sees
        torch.cuda.synchronize()
        ts = time.perf_counter()
        marks = [ts]
        for _ in range(args.steps):
            step(False)
            marks.append(time.perf_counter())
        torch.cuda.synchronize()
        synced_ms = (time.perf_counter() - ts) / args.steps * 1e3
        step_ms = [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]
    if two:
        # the multi-context loop (after W warm-up jobs of its own): K jobs alternating between the
        # engines.  A plain run's only loop; with --full the third
        eng.enable_timing(0)
        for i in range(args.warmup):
            step2(i)
        drain2()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for i in range(args.steps):
            step2(i)
        drain2()                                  # every job's read-back (errors surface here)
        torch.cuda.synchronize()
        two_ms = (time.perf_counter() - t2) / args.steps * 1e3
        last = engs[(args.steps - 1) % len(engs)]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last.result())
    stats = eng.stats()
    # --full: every phase (events around each), on instrumented steps after the timed region; N > 1 also
    # times the step's stages on the host clock with a synchronise after each (the shuffle through
    # gloo, host-staged, has no engine events; RCCL's wcg_exchange / wcg_gather_merge have them)
    psteps = max(1, min(args.steps, 10)) if full else 0
    eng.enable_timing(2 if full else 0)
    wall = {"map": 0.0, "shuffle": 0.0, "owner_reduce": 0.0, "gather_merge": 0.0}
    map_stats = None
    for _ in range(psteps):
        if world == 1:
            step()
            continue
        t0p = time.perf_counter()
        eng.reset()
        eng.map_device(dev.data_ptr(), n)
        torch.cuda.synchronize()
        t1p = time.perf_counter()
        if map_stats is None:                     # this rank's map counters (the owners' jobs reset them)
            map_stats = eng.stats()
            t1p = time.perf_counter()
        wd.shuffle(teng, args.nreduce)
        torch.cuda.synchronize()
        t2p = time.perf_counter()
        teng.reduce()
        torch.cuda.synchronize()
        t3p = time.perf_counter()
        wd.gather_merge(teng, fetch=False)
        torch.cuda.synchronize()
        t4p = time.perf_counter()
        for k, a, b in (("map", t0p, t1p), ("shuffle", t1p, t2p), ("owner_reduce", t2p, t3p),
                        ("gather_merge", t3p, t4p)):
            wall[k] += (b - a) * 1e3
    ph_sum = eng.timings()[0] if full else {}
    eng.enable_timing(0)
    if world > 1:                                 # every rank's counters and (--full) phase times
        per_rank = [None] * world
        mine = {"stats": stats, "step_ms": step_ms}
        if full:
            mine.update({"phase_ms_avg": {k: round(v / psteps, 4) for k, v in ph_sum.items()},
                         "phase_wall_ms_avg": {k: round(v / psteps, 4) for k, v in wall.items()},
                         "map_stats": map_stats})
        dist.all_gather_object(per_rank, mine)

    # ---- --full: verify the last step's output against the oracle (outside the timed region)
    verified = None
    if full and not args.no_verify:
        from tests import oracle_bridge as ob
        data = host.numpy().tobytes()
        if world == 1:
            want = ob.merged(data, 16)
            verified = all(e.result() == want for e in engs)   # several contexts: every engine's last job
        else:
            # every rank counts its own range with the oracle; root sums the counts of all ranks
            # and compares the merged file the GPUs left in root's HBM
            mine = ob.merged(data, 16)
            parts = [None] * world if rank == 0 else None
            dist.gather_object(mine, parts, dst=0)
            ok = [None]
            if rank == 0:
                from tests.oracle_bridge import wc_ref
                tot = {}
                for p in parts:
                    for line in p.splitlines():
                        k, c = line.rsplit(b": ", 1)
                        tot[k] = tot.get(k, 0) + int(c)
                ok[0] = eng.result() == wc_ref.merged_output(tot)
            dist.broadcast_object_list(ok, src=0)
            verified = ok[0]
        del data
        if not verified:
            sys.stderr.write("bench: GPU result differs from the oracle; refusing to report a rate\n")
            sys.exit(3)

    if rank == 0:
        # N = 1 with --full: two or three K-step loops ran the same full jobs (contexts: jobs dealt in
        # turn to --contexts engines on their own streams; pipelined: reset, map, wcg_reduce_async back
        # to back on one engine; synced: every job waits for its reduce's read-back), each bracketed
        # by torch.cuda.synchronize(); the fastest is the value and step_mode names it (between two
        # boxes the synced loop was the faster of the one-engine loops by 0.9 % on one, the
        # pipelined one by 1.7 % on the other).  A plain run has one loop, and it is the value.
        if dt is None:
            ms_step, mode_used = two_ms, "contexts"
        else:
            ms_step, mode_used = dt / args.steps * 1e3, "pipelined" if pipe else "synced"
        ms_pipelined = ms_step if pipe else None
        if synced_ms is not None and synced_ms < ms_step:
            ms_step, mode_used = synced_ms, "synced"
        if two_ms is not None and two_ms < ms_step:
            ms_step, mode_used = two_ms, "contexts"
        dt = ms_step * args.steps / 1e3
        all_bytes = total if strong else n * world
        gbs = all_bytes / (dt / args.steps) / 1e9
        # HIP events over the one-engine loop's timed steps (a plain multi-context run has none)
        avg_map_ms = map_sum["map"] / args.steps if map_sum is not None else 0.0
        achieved = n / (avg_map_ms * 1e-3) / 1e9 if avg_map_ms > 0 else None
        traffic = None
        try:
            with open(args.traffic_json) as f:
                tj = json.load(f)
            if tj.get("bytes_per_gpu") == n and tj.get("workload") == workload:
                traffic = tj.get("hbm_bytes_per_launch")
        except (OSError, ValueError):
            pass
        out = {
            "metric": "word-count input GB/s (whole node) and % of HBM roofline at 1/2/4/8 MI355X",
            "value": round(gbs, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic (csrc/gencorpus.c; kjv12.txt absent)",
            "config": {"workload": workload, "total_bytes": all_bytes, "bytes_per_gpu": n, "vocab": cfg["vocab"],
                       "zipf_s": cfg["zipf_s"], "seed": cfg["seed"], "nreduce": args.nreduce,
                       "hbm_roofline_frac_whole_step": round(gbs / (HBM_PEAK_GBS * world), 4),
                       "parallelism": f"{world} ranks, one line-aligned range each",
                       "shuffle": None if world == 1 else
                       ("gloo rehearsal, host-staged" if gloo else
                        "wcg_exchange: RCCL allgather of the count rows, grouped ncclSend/ncclRecv of the "
                        "32-byte units; owners sort; wcg_gather_merge: runs to rank 0, k-way merge")},
            "roofline": {"bound": "hbm", "kernel": "wcg::k_map",
                         "achieved": round(achieved, 2) if achieved else None,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
                         "traffic": traffic, "avg_launch_ms": round(avg_map_ms, 4),
                         "algorithmic_bytes_per_launch": n,
                         "measured_on": "HIP events around every k_map launch of the one-engine pipelined loop "
                                        "(each launch alone on the GPU; in the multi-context loop two jobs' "
                                        "kernels share the CUs)" if pipe else
                                        "HIP events around every k_map launch of the timed loop"},
        }
        out["full"] = full
        if map_sum is None:                       # a plain multi-context run: no events around k_map
            del out["roofline"]
        # per-step spread (host clock between steps; N > 1: each step's slowest rank); N = 1 with
        # pipelined jobs: from the synced loop of --full
        if world > 1:
            srt = sorted(max(v) for v in zip(*[r["step_ms"] for r in per_rank]))
        else:
            srt = sorted(step_ms)

        def q(f):
            return round(srt[min(len(srt) - 1, int(f * (len(srt) - 1) + 0.5))], 4)
        if srt:
            out["ms_per_step_median"] = q(0.5)
            out["ms_per_step_spread"] = {"min": q(0.0), "p10": q(0.1), "p90": q(0.9), "max": q(1.0),
                                         "how": ("host clock between the steps of a second K-step loop in which "
                                                 "every step waits for its reduce (wcg_reduce); value uses the "
                                                 "mean over the fastest of the bracketed loops (step_mode)" if pipe else
                                                 "host clock between steps (each step ends in a host wait); "
                                                 "value uses the mean over the bracketed loop")}
            out["value_at_median_step"] = round(all_bytes / (q(0.5) * 1e-3) / 1e9, 3)
        out["step_mode"] = {
            "contexts": f"{nctx} contexts: jobs dealt in turn to {nctx} engines, each on its own stream and "
                        "hardware queue (reset, map, wcg_reduce_async; an engine's previous job is waited for "
                        "before its reuse), so one job's map runs on the CUs another's aggregation tail and "
                        "reduce leave idle; every job runs in full, every engine's last output verified "
                        "(--full); the last jobs' read-backs waited for inside the timed region",
            "pipelined": "pipelined: reset, map, wcg_reduce_async per job, back to back on one stream; the last "
                         "job's read-back waited for inside the timed region",
            "synced": "synchronous: each job ends in its reduce's host read-back (wcg_reduce)"}[mode_used]
        if two_ms is not None:
            out["loop_order"] = ("after W warm-up jobs: the pipelined loop (the first, so it carries the GPU's "
                                 "clock ramp from idle), the synced loop, then W more warm-up jobs and the "
                                 "multi-context loop" if full else
                                 "W warm-up jobs, then the K timed jobs, all in the multi-context loop")
            out["contexts"] = nctx
            out["ms_per_step_contexts"] = round(two_ms, 4)
            out["value_contexts"] = round(all_bytes / (two_ms * 1e-3) / 1e9, 3)
        if synced_ms is not None:
            out["ms_per_step_pipelined"] = round(ms_pipelined, 4)
            out["value_pipelined"] = round(all_bytes / (ms_pipelined * 1e-3) / 1e9, 3)
            out["ms_per_step_host_synced"] = round(synced_ms, 4)
            out["value_host_synced"] = round(all_bytes / (synced_ms * 1e-3) / 1e9, 3)
        out["stats"] = stats
        if full:
            out["phase_ms_avg"] = {k: round(v / psteps, 4) for k, v in ph_sum.items()
                                   if world > 1 or k in ("map", "agg", "compact", "sort", "format")}
            out["phase_timing"] = (f"HIP events around every phase on {psteps} instrumented steps after the "
                                   "timed region (the timed steps carry events around k_map only)")
        if world == 1:
            fused = eng.reduce_path() == 1
            out["reduce_path"] = ("one launch (csrc/wcg_fused.h): compaction, sort and formatting in one "
                                  "persistent kernel, reported as phase 'sort'" if fused else "multi-launch")
        if world > 1:
            # the N > 1 step by phase (device time on each rank's work stream, HIP events):
            # map/agg/compact/sort/format = the rank's own map + its owners' DoReduce;
            # export (compaction, unit counts, counts all-to-all + its host read, unit writes),
            # exchange (RCCL send/recv of the units), import, gather (RCCL runs -> rank 0),
            # merge (k-way merge of the runs at rank 0)
            out["per_rank"] = per_rank
        if world > 1 and full:
            out["phase_ms_avg_max_over_ranks"] = {
                k: max(r["phase_ms_avg"][k] for r in per_rank) for k in per_rank[0]["phase_ms_avg"]}
            out["phase_wall_ms_avg_max_over_ranks"] = {
                k: max(r["phase_wall_ms_avg"][k] for r in per_rank) for k in per_rank[0]["phase_wall_ms_avg"]}
        out["verified_vs_oracle"] = verified
        if full and world == 1 and not args.no_end_to_end:
            out["end_to_end"] = end_to_end(keys_cap, cfg, n)
        if full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"], out["cpu_baseline_parallel"], out["cpu_restatement_all_cores"] = \
                cpu_baselines(cfg, args.cpu_sample_mib << 20)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
