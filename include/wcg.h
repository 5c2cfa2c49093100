/*
 * wcg.h - C ABI of the MI355X word-count engine (libwcg.so).
 *
 * This is the drop-in boundary for the Lab 1 MapReduce word-count hot path of
 * wushan270/mit-6.824-2015.  The reference's "plugin API" is a pair of Go function values,
 *   Map    func(string) *list.List              (/root/reference/src/main/wc.go:17)
 *   Reduce func(string, *list.List) string      (/root/reference/src/main/wc.go:35)
 * run by the data plane of package mapreduce
 *   RunSingle  mapreduce.go:344-356   Split 141-179   DoMap 193-231   ihash 185-189
 *   DoReduce   mapreduce.go:239-280   Merge 284-321   MapName/ReduceName/MergeName 136,181,233
 * and by the worker RPC handler Worker.DoJob (worker.go:22-34).
 *
 * A GPU backend must implement Map AND Reduce together (the device pre-aggregates
 * (key, count) pairs, which the per-occurrence CPU Reduce = len(list) could not consume),
 * so the ABI is phase-shaped - one C call per phase, never one per token:
 *
 *   wcg_open     ~ InitMapReduce for a wc job on one GPU            (mapreduce.go:68-82)
 *   wcg_map*     ~ DoMap(job) + Map over one split's bytes           (mapreduce.go:193-231)
 *   wcg_reduce   ~ all DoReduce jobs + Merge: sorted "key: count\n"  (mapreduce.go:239-321)
 *   wcg_partition~ DoReduce(job=r) output bytes mrtmp.<f>-res-<r>    (mapreduce.go:264-279)
 *   wcg_export / wcg_import ~ the ihash%nReduce shuffle (mapreduce.go:214-230 + 242-263),
 *                  done as an all-to-all-v of pre-aggregated records between GPUs.
 *   wcg_map_file ~ Split + DoMap x nMap from the input file (mapreduce.go:141-179, 193-231)
 *   wcg_merge_runs ~ Merge of the owners' sorted DoReduce outputs  (mapreduce.go:284-321)
 *   wcg_map_json ~ DoMap's per-occurrence JSON intermediates       (mapreduce.go:214-230)
 *   wcg_index_merged / wcg_load_merged ~ the merged file mrtmp.<f> made searchable (test-wc.sh:2-3
 *                  asks its question of that file)
 *   wcg_import_json ~ DoReduce's and Merge's reading of the JSON files (mapreduce.go:242-263,
 *                  289-303): mrtmp.<f>-<m>-<r> and mrtmp.<f>-res-<r> decoded on the device
 *
 * Conventions:
 *   - Every entry point returns int status (WCG_OK = 0); the host turns non-zero into a fatal
 *     error exactly where the reference calls log.Fatal.  wcg_last_error() explains it.
 *   - Output buffers are library-owned (valid until the next call on the same context).
 *   - The library never retains caller pointers past a call.
 *   - Every entry point makes the context's device current (the HIP current device is
 *     per host thread; Go goroutines migrate between threads).
 *   - A context is not thread-safe.
 */
#ifndef WCG_H
#define WCG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef WCG_API
#define WCG_API __attribute__((visibility("default")))
#endif

typedef struct wcg_ctx wcg_ctx;

enum {
    WCG_OK = 0,
    WCG_EINVAL = 1,   /* bad argument                                                */
    WCG_ENOMEM = 2,   /* device allocation failed                                    */
    WCG_EHIP = 3,     /* HIP runtime error                                           */
    WCG_EFULL = 4,    /* aggregation table overflowed (max_keys too small)           */
    WCG_ESTATE = 5    /* call out of order (e.g. wcg_partition before wcg_reduce)    */
};

enum {
    WCG_FMT_MERGED = 0,    /* "key: count\n", all keys, bytewise order  (Merge output)   */
    WCG_FMT_RES_JSON = 1   /* {"Key":"k","Value":"count"}\n for ihash(k)%R == r          */
};

/* Open a context on HIP device `device`.
 *   max_input_bytes: a hint (kept for ABI compatibility): wcg_map streams splits of any size
 *                    through fixed pinned staging buffers; 0 is fine
 *   max_keys:        capacity in distinct keys of the device aggregation table */
WCG_API int wcg_open(int device, uint64_t max_input_bytes, uint64_t max_keys, wcg_ctx **out);
WCG_API int wcg_close(wcg_ctx *ctx);
WCG_API const char *wcg_last_error(const wcg_ctx *ctx);

/* Run all device work of this context on `stream` (a hipStream_t; NULL = the context's own
 * stream).  Lets a host framework time the phases with its own events. */
WCG_API int wcg_set_stream(wcg_ctx *ctx, void *stream);

/* Forget all aggregated keys (start a new job). */
WCG_API int wcg_reset(wcg_ctx *ctx);

/* DoMap + Map (mapreduce.go:193-231, wc.go:17-30) over one split held in host memory:
 * copy to HBM, tokenize into maximal unicode.IsLetter runs, aggregate (key, count).
 * Splits must be cut where a token cannot straddle (Split cuts at '\n').  Large splits are
 * streamed in chunks (cut after an ASCII non-letter) through pinned double buffers, so the
 * copy of one chunk overlaps the map of the previous one.  Returns once host_bytes has been
 * consumed (the caller may free it); the device work is asynchronous. */
WCG_API int wcg_map(wcg_ctx *ctx, const uint8_t *host_bytes, uint64_t n);

/* Same, input already resident in device memory (n bytes at dev_bytes). Asynchronous. */
WCG_API int wcg_map_device(wcg_ctx *ctx, const void *dev_bytes, uint64_t n);

/* The size limit of one wcg_map_device call (pure arithmetic, no device): the map kernel counts
 * its 992-byte steps in 32 bits, so a split of about 4 TB or more is WCG_EINVAL (wcg_map_device
 * checks this before it looks at the pointer or the device); anything smaller is WCG_OK. */
WCG_API int wcg_map_size_check(uint64_t n);

/* Split (mapreduce.go:141-179) + DoMap x nMap over a whole input file, on the GPU: the file is
 * read by a pool of host threads into two pinned staging buffers and copied to HBM in
 * line-aligned chunks, each copy overlapping the map kernels of the previous chunk.  Split's
 * quirk P1 is kept: the first line that does not fit bufio.Scanner's 64 KiB buffer together with
 * its '\n' ends the input (the reference's scan stops there silently).  *mapped_bytes = bytes
 * counted (the whole file unless P1 cut it), *file_bytes = file size.  Asynchronous. */
WCG_API int wcg_map_file(wcg_ctx *ctx, const char *path, uint64_t *mapped_bytes, uint64_t *file_bytes);

/* DoReduce x nReduce + Merge (mapreduce.go:239-321): sort all keys bytewise on the device and
 * format the merged file "key: count\n".  Synchronous; returns key count and byte size. */
WCG_API int wcg_reduce(wcg_ctx *ctx, uint64_t *nkeys, uint64_t *nbytes);

/* The same job without the host wait: the reduce is queued on the context's stream (with the
 * read-back of its sizes and error flags) and the call returns at once, so a host can queue the
 * next job's wcg_reset / wcg_map* behind it (back-to-back jobs then run without host gaps).
 * wcg_reduce_wait returns what wcg_reduce would have (sizes, or the job's error); every call that
 * reads the job's results (wcg_result_*, wcg_partition*, wcg_export*, wcg_stats, wcg_timings,
 * wcg_sync, the collectives) waits for it first.  A job not waited for before the next wcg_reset
 * / wcg_map / wcg_map_device / wcg_map_file / wcg_import is dropped, its results and its error
 * status with it (wcg_map_json aggregates nothing and leaves the job alone; wcg_import_json drops
 * it when it accepts its file and leaves it alone when it refuses it).  Jobs that take
 * the multi-launch reduce (the first job of a context, large or two-pass jobs) are reduced
 * synchronously here as by wcg_reduce. */
WCG_API int wcg_reduce_async(wcg_ctx *ctx);
WCG_API int wcg_reduce_wait(wcg_ctx *ctx, uint64_t *nkeys, uint64_t *nbytes);

/* Device pointer to / host copy of the formatted output of the last wcg_reduce(). */
WCG_API int wcg_result_device(wcg_ctx *ctx, const void **dev_ptr, uint64_t *nbytes);
WCG_API int wcg_result_copy(wcg_ctx *ctx, uint8_t *host_out, uint64_t cap);
/* Device-to-device copy of that output (nbytes of wcg_reduce) into dev_dst, asynchronous on the
 * context's stream (e.g. into a collective's send buffer). */
WCG_API int wcg_result_copy_device(wcg_ctx *ctx, void *dev_dst);

/* Wait for all device work queued on the context's stream. */
WCG_API int wcg_sync(wcg_ctx *ctx);

/* Release a library-owned device buffer before the context is closed: the formatted output of
 * wcg_result_device() or the records of wcg_export() (output buffers are
 * library-owned until wcg_free).  Waits for the context's stream first.  Afterwards the result
 * calls report WCG_ESTATE until the next wcg_reduce(); a later call that needs the buffer
 * allocates it again.  Any other pointer: WCG_EINVAL. */
WCG_API int wcg_free(wcg_ctx *ctx, const void *dev_ptr);

/* Bytes of mrtmp.<f>-res-<r> (DoReduce output, mapreduce.go:264-279) for partition r of
 * nreduce, in sorted key order, copied to host_out (cap bytes).  *nbytes gets the size;
 * host_out == NULL queries the size only.  Requires a prior wcg_reduce(). */
WCG_API int wcg_partition(wcg_ctx *ctx, uint32_t nreduce, uint32_t r, uint8_t *host_out, uint64_t cap,
                  uint64_t *nbytes);

/* Every DoReduce output file at once: the nreduce -res-<r> files back to back in partition order
 * (one formatting pass for all of them; nreduce <= 1024).  part_bytes[nreduce] gets each file's
 * size; host_out == NULL queries the sizes only (the files stay cached on the device until the
 * next job, so wcg_partition of any r is then a copy). */
WCG_API int wcg_partition_all(wcg_ctx *ctx, uint32_t nreduce, uint8_t *host_out, uint64_t cap,
                              uint64_t *part_bytes);

/* The n most frequent words: the bytes that `LC_ALL=C sort -n -k2 <merged file> | tail -n <n>`
 * prints for the merged file of the last wcg_reduce() - the reference's acceptance check of word
 * count (src/main/test-wc.sh:2-3, with n = 10, diffed against mr-testout.txt).  Lines
 * "key: count\n", ascending by count (compared as unsigned 64-bit), lines of equal count ascending
 * by bytewise key, the last min(n, keys) of that order; selected and formatted on the device from
 * the sorted records, so only those lines cross to the host.  *nlines / *nbytes get their number
 * and size; host_out == NULL queries them only (the lines stay cached on the device for this n
 * until the next job, so a second call with the same n is a copy).  n == 0: no lines;
 * n > WCG_TOP_MAX: WCG_EINVAL (take the merged file).  Requires a prior wcg_reduce() (a pending
 * wcg_reduce_async job is waited for): WCG_ESTATE before one, after wcg_free of its result, and
 * after wcg_merge_runs / wcg_gather_merge* on the context that holds the merged file (its records
 * are lines without counts) until wcg_index_merged has made query records of them; without that
 * call, wcg.top_merge in Python combines the ranks' tops on the host.  The result
 * calls, wcg_partition*, wcg_export*, wcg_stats and wcg_timings in between do not disturb it (they
 * leave the sorted records alone; should an export ever have to regrow the record buffers,
 * wcg_top reports WCG_ESTATE rather than read freed records). */
#define WCG_TOP_MAX 1024
WCG_API int wcg_top(wcg_ctx *ctx, uint32_t n, uint8_t *host_out, uint64_t cap, uint64_t *nlines,
                    uint64_t *nbytes);

/* "How often does this word occur?"  counts[i] = the count of key i in the last wcg_reduce()'s
 * result, 0 if it does not occur: a binary search per key over the sorted records on the device,
 * so only the counts cross to the host.  Key i is the bytes keys[key_off[i] .. key_off[i+1])
 * (key_off has nq + 1 entries, non-decreasing, key_off[0] == 0; otherwise WCG_EINVAL).  Any bytes
 * are allowed: an empty key, a key holding a NUL or 0xFF byte or a non-letter simply does not
 * occur.  nq == 0 is WCG_OK and touches nothing.  State rules as wcg_top's: WCG_ESTATE before a
 * wcg_reduce() (a pending wcg_reduce_async job is waited for), after wcg_free of its result and
 * after wcg_merge_runs / wcg_gather_merge* (until wcg_index_merged); the result calls, wcg_partition*, wcg_export*, wcg_top,
 * wcg_stats and wcg_timings in between do not disturb it.  After wcg_exchange every key has one
 * owner, so a word's count over all ranks is the sum of the ranks' lookups. */
WCG_API int wcg_lookup(wcg_ctx *ctx, const uint8_t *keys, const uint64_t *key_off, uint64_t nq,
                       uint64_t *counts);

/* The same with keys, offsets and counts in device memory; asynchronous on the context's stream
 * (the offsets are not checked). */
WCG_API int wcg_lookup_device(wcg_ctx *ctx, const void *dev_keys, const void *dev_key_off, uint64_t nq,
                              void *dev_counts);

/* The lines "key: count\n" of the merged file with lo <= key < hi (bytewise), in file order,
 * found and formatted on the device.  lo == NULL: from the first line; hi == NULL: to the last.
 * lo >= hi: no lines (WCG_OK).  *nlines / *nbytes are always set; host_out == NULL queries them
 * only (the lines stay cached on the device until the next job, so a second call whose bounds
 * select the same lines is a copy); cap < *nbytes: WCG_EINVAL.  State rules as wcg_lookup's. */
WCG_API int wcg_range(wcg_ctx *ctx, const uint8_t *lo, uint64_t lo_len, const uint8_t *hi, uint64_t hi_len,
                      uint8_t *host_out, uint64_t cap, uint64_t *nlines, uint64_t *nbytes);

/* The merged file in count order: its lines as `LC_ALL=C sort -n -k2 <merged file>` prints them
 * (test-wc.sh:2-3 without the tail) - ascending by count (compared as unsigned 64-bit), lines of
 * equal count ascending by bytewise key, a prefix before its extensions.  With K the keys of the
 * result (what wcg_reduce / wcg_index_merged report), rank 0 is the first line of that output and
 * rank K-1 the most frequent word.  The order is sorted on the device from the sorted records (a
 * radix sort of (count, record index): no key byte is compared), on the first of these calls after
 * a result and kept until the next job; wcg_reduce itself launches what it always did.
 *   wcg_by_count: the lines at ranks [first, min(first + n, K)) to host_out.  first + n saturates
 * (n = UINT64_MAX: to the end); first >= K or n == 0: no lines (WCG_OK).  *nlines / *nbytes are
 * always set; host_out == NULL queries them only (the window's lines stay cached on the device
 * until the next job, so a second call that selects the same lines is a copy); cap < *nbytes:
 * WCG_EINVAL.  For every n <= WCG_TOP_MAX, wcg_by_count(K - min(n, K), n) gives wcg_top(n)'s bytes.
 *   wcg_by_count_device: the same lines left in a library-owned device buffer (*dev_ptr; NULL when
 * there are none).  It is the window cache: valid until the next wcg_by_count* call with another
 * window or the next job, freed by wcg_close; wcg_free does not take it.
 *   wcg_count_rank: ranks[i] = the number of keys whose count is below counts[i] (0 .. K), a binary
 * search per count on the device.  The keys with a count >= c are the ranks [rank(c), K), those
 * with exactly c the ranks [rank(c), rank(c + 1)).  nq == 0 is WCG_OK and touches nothing; a NULL
 * pointer with nq > 0: WCG_EINVAL.
 * State rules as wcg_lookup's (after wcg_index_merged / wcg_load_merged* the calls work as after
 * wcg_reduce); the result calls, wcg_partition*, wcg_export*, wcg_top, wcg_lookup*, wcg_range,
 * wcg_stats and wcg_timings in between do not disturb the order.  A device allocation that fails
 * is WCG_ENOMEM, and the result and its other queries stay as they were.  The order names a record
 * by a 32-bit index: a result of 2^32 sorted records or more is WCG_EINVAL, checked before
 * anything is launched. */
WCG_API int wcg_by_count(wcg_ctx *ctx, uint64_t first, uint64_t n, uint8_t *host_out, uint64_t cap,
                         uint64_t *nlines, uint64_t *nbytes);
WCG_API int wcg_by_count_device(wcg_ctx *ctx, uint64_t first, uint64_t n, const void **dev_ptr,
                                uint64_t *nlines, uint64_t *nbytes);
WCG_API int wcg_count_rank(wcg_ctx *ctx, const uint64_t *counts, uint64_t nq, uint64_t *ranks);

/* Diagnostics: the last build of the count order.  out[0] = the context holds an order, out[1] =
 * the digit passes it ran (bit d: the pass over byte d of the counts; a byte in which all counts
 * agree is skipped), and, when wcg_enable_timing was on during the build, device milliseconds:
 * out[2] the pass that reads the records, out[3 + d] the pass of digit d (0: skipped).
 * n = number of doubles the caller provides (<= 11). */
WCG_API int wcg_by_count_stats(wcg_ctx *ctx, double *out, int n);

/* DoMap's reference-exact intermediate files (mapreduce.go:214-230) for one split: for every
 * token, in input order, the line {"Key":"tok","Value":"1"}\n in file ihash(tok) % nreduce - the
 * bytes the reference's json.Encoder writes to mrtmp.<f>-<m>-<r>, so an unmodified CPU DoReduce
 * can consume GPU map output.  Files back to back in partition order; part_bytes[nreduce] gets
 * each size; host_out == NULL queries the sizes only; cap < the files' total: WCG_EINVAL.
 * nreduce <= 1024, as for wcg_partition_all: 0 or more is WCG_EINVAL, checked before anything is
 * allocated, copied or launched (the split is walked once per 128 partitions).  Independent of the
 * aggregation tables: the call neither reads nor changes the keys mapped so far, the last
 * wcg_reduce()'s result or what wcg_partition*, wcg_top, wcg_lookup and wcg_range cache of it, and
 * it is not one of the wcg_map* calls that drop a pending wcg_reduce_async job (it only waits for
 * the stream the job runs on; wcg_reduce_wait then returns the job's sizes as usual). */
WCG_API int wcg_map_json(wcg_ctx *ctx, const uint8_t *host_bytes, uint64_t n, uint32_t nreduce,
                         uint8_t *host_out, uint64_t cap, uint64_t *part_bytes);

/* ---- multi-GPU shuffle (one process per GPU; the host moves the buffers with RCCL) ----
 * wcg_export: bucket the local aggregate by owner = (ihash(key) % nreduce) % nranks into a
 * device buffer of fixed 32-byte records (long keys > 15 bytes are carried in following
 * 32-byte continuation records).  counts[nranks] receives records per destination, in order.
 * wcg_import: aggregate records received from peers into this context's table (call after
 * wcg_reset() on the receiving side, or onto a live table). */
#define WCG_RECORD_BYTES 32
WCG_API int wcg_export(wcg_ctx *ctx, uint32_t nreduce, uint32_t nranks, const void **dev_records,
               uint64_t *counts);
WCG_API int wcg_import(wcg_ctx *ctx, const void *dev_records, uint64_t nrecords);

/* The same export in two steps, writing straight into a caller's device buffer (e.g. the send
 * buffer of an RCCL all-to-all-v): wcg_export_count returns the units per destination rank
 * (one host synchronisation); wcg_export_write then fills dev_dst (sum(counts) units, rank
 * order) asynchronously on the context's stream.  wcg_import is asynchronous too: a table that
 * filled is reported by the next wcg_reduce / wcg_export_count. */
WCG_API int wcg_export_count(wcg_ctx *ctx, uint32_t nreduce, uint32_t nranks, uint64_t *counts);
WCG_API int wcg_export_write(wcg_ctx *ctx, void *dev_dst);

/* ---- the shuffle and the final Merge inside the library, over RCCL (one process per GPU) ----
 * The reference moves partitions between its phases as files: DoMap writes mrtmp.<f>-<m>-<r>
 * for r = ihash(key) % nReduce (mapreduce.go:214-230), DoReduce r reads partition r of every
 * map job (mapreduce.go:242-263), Merge reads every -res-<r> (mapreduce.go:284-321).  On one
 * node of GPUs these hand-offs are RCCL collectives over xGMI on the context's stream:
 *   wcg_comm_id      ncclGetUniqueId: made on rank 0, handed to every rank by the host (the
 *                    config-5 master RPC, torch.distributed, a file - 128 opaque bytes)
 *   wcg_comm_init    ncclCommInitRank for this context (world may be 1)
 *   wcg_exchange     export the local aggregate by owner = (ihash % nreduce) % world into a send
 *                    buffer, ncclAllGather every rank's row {status, buffer capacities, units per
 *                    owner}, ONE host read of that world x world matrix, the plan of
 *                    wcg_exchange_plan, grouped ncclSend/ncclRecv of the 32-byte units, then this
 *                    context keeps exactly the keys of the partitions it owns (tables cleared,
 *                    received units imported).  All device work is ordered on the context's
 *                    stream; *sent / *received = units (may be NULL).  Follow with wcg_reduce
 *                    (DoReduce of the owned partitions: sorted "key: count" run of this rank).
 *   wcg_gather_merge after wcg_reduce on every rank: every rank's sorted run goes to `root`
 *                    (ncclAllGather of {status, run size, capacity}, one host read,
 *                    ncclSend/ncclRecv, placement of wcg_gather_plan), which merges the runs on
 *                    its GPU (as wcg_merge_runs) into its result.  On root *nkeys / *nbytes
 *                    describe the merged file; elsewhere they are 0.
 * Collective calls: every rank of the communicator makes them in the same order.  A rank that
 * fails before data moves (a full table: WCG_EFULL; a call out of order; an allocation) still
 * joins the collectives with its status, and then EVERY rank returns an error (no rank is left
 * waiting in a send or receive); no units have moved and the tables are as they were.  A device
 * fault (a sticky HIP error: the context's stream can run nothing more, collectives included) is
 * outside this contract: that rank cannot join, its peers wait in the collective until the job is
 * stopped (bench.py's launcher stops every rank after --launch-timeout).  wcg_exchange_local
 * applies the same agreement across its contexts (tests/test_gpu_exchange_local.py forces a full
 * table on one of them). */
#define WCG_COMM_ID_BYTES 128
WCG_API int wcg_comm_id(uint8_t *id_out /* WCG_COMM_ID_BYTES */);
WCG_API int wcg_comm_init(wcg_ctx *ctx, const uint8_t *id /* WCG_COMM_ID_BYTES */, int rank, int world);
WCG_API int wcg_exchange(wcg_ctx *ctx, uint32_t nreduce, uint64_t *sent, uint64_t *received);
WCG_API int wcg_gather_merge(wcg_ctx *ctx, int root, uint64_t *nkeys, uint64_t *nbytes);

/* The host-side plan of the shuffle and of Merge's gather (pure arithmetic, no device; what
 * wcg_exchange / wcg_gather_merge compute from the gathered counts).
 *   wcg_exchange_plan: counts[s * world + d] = units rank s sends to rank d.  For `rank`:
 *     send_off[d] / send_cnt[d] = where its units for d start in its send buffer and how many;
 *     recv_off[s] / recv_cnt[s] = where the units from s land in its receive buffer (source-rank
 *     order); totals[2] = {units sent, units received}.  Output arrays may be NULL.
 *   wcg_gather_plan: sizes[p] = bytes of rank p's sorted run; run_off[p] = where it lands in
 *     root's receive buffer (root's own run is copied to run_off[root]); *total = all bytes. */
WCG_API int wcg_exchange_plan(const uint64_t *counts, uint32_t world, uint32_t rank, uint64_t *send_off,
                              uint64_t *send_cnt, uint64_t *recv_off, uint64_t *recv_cnt, uint64_t *totals);
WCG_API int wcg_gather_plan(const uint64_t *sizes, uint32_t world, uint32_t root, uint64_t *run_off,
                            uint64_t *total);

/* The same shuffle and Merge across `world` contexts of ONE process (e.g. several contexts on one
 * GPU standing in for the ranks of a node): the count matrix, the plans above, the export, import
 * and merge kernels are wcg_exchange's and wcg_gather_merge's; device-to-device copies stand in
 * for the RCCL sends and receives.  sent[world] / received[world] get each context's units. A
 * test transport for world > 1 where one GPU cannot host several RCCL ranks. Synchronous. */
WCG_API int wcg_exchange_local(wcg_ctx **ctxs, uint32_t world, uint32_t nreduce, uint64_t *sent,
                               uint64_t *received);
WCG_API int wcg_gather_merge_local(wcg_ctx **ctxs, uint32_t world, uint32_t root, uint64_t *nkeys,
                                   uint64_t *nbytes);

/* Merge (mapreduce.go:284-321) of sorted runs: dev_text holds nruns formatted outputs back to
 * back (each a sorted "key: count\n" file, e.g. the wcg_reduce output of every owner rank, with
 * disjoint keys), run r being run_bytes[r] bytes.  The runs are merged pairwise on the device
 * (ceil(log2 nruns) merge passes, long-key ties by full bytes) into this context's result
 * (wcg_result_device / wcg_result_copy).  Synchronous. */
WCG_API int wcg_merge_runs(wcg_ctx *ctx, const void *dev_text, const uint64_t *run_bytes, uint32_t nruns,
                           uint64_t *nkeys, uint64_t *nbytes);

/* Query a merged file.  wcg_index_merged builds, on the device, the records wcg_top, wcg_lookup,
 * wcg_lookup_device and wcg_range search, for the merged file this context holds: valid after
 * wcg_merge_runs, wcg_gather_merge* (on the root) and wcg_load_merged*.  Every line is checked on
 * the way (wcg.check_merged states the rules in Python); per line, in this order:
 *   count  the line is key, ": ", a canonical decimal in 1 .. 2^64-1 (first digit 1-9, at most 20
 *          digits), '\n'; the key is not empty and ends at the line's first ':'
 *   zero   the count is not "0"
 *   nul    the key holds no zero byte
 *   order  the key sorts strictly after the previous line's (bytewise, a prefix first): equal
 *          adjacent keys are rejected (the runs of a merge have disjoint keys by contract)
 * A file that breaks a rule: WCG_EINVAL, and wcg_last_error() reads
 * "wcg_index_merged: line <N>: <rule> (...)" for the first such line (N counts from 0); the
 * wcg_result_* calls still return the merged bytes and the queries stay WCG_ESTATE.  Afterwards
 * the queries work exactly as after wcg_reduce, with the same caches; *nlines = the file's lines.
 * Synchronous.  A second call, or a call on a context whose result came from wcg_reduce (*nlines =
 * its key count), does nothing and returns WCG_OK; before any result: WCG_ESTATE.  An empty merged
 * file indexes to zero records (lookups give zeros, top and range no lines).  The merged file is
 * the records' key storage: wcg_free of the result buffer drops the index (queries are WCG_ESTATE
 * again), as wcg_reset, wcg_map*, wcg_import, a new merge and wcg_reduce drop any result.
 * wcg_partition*, wcg_export*, wcg_exchange* and wcg_gather_merge* on a merged context stay
 * WCG_ESTATE, indexed or not.  Without the call nothing changes: wcg_merge_runs launches what it
 * always did. */
WCG_API int wcg_index_merged(wcg_ctx *ctx, uint64_t *nlines);

/* One sorted "key: count\n" file (yesterday's mrtmp.<file>, or one the CPU reference wrote) into
 * this context as its merged result, indexed: wcg_merge_runs with one run (except that the file is
 * checked, not trusted: no line is moved), then wcg_index_merged.  The host form copies the file
 * to the device through the context's pinned staging buffers.  n > 0 with a last byte other than
 * '\n' is WCG_EINVAL ("newline" in wcg_last_error), checked before anything is copied or launched
 * (the host form: before the device is touched; the device form reads that one byte first).  Like
 * wcg_merge_runs they drop a pending wcg_reduce_async job and are synchronous. */
WCG_API int wcg_load_merged(wcg_ctx *ctx, const uint8_t *host_bytes, uint64_t n, uint64_t *nlines);
WCG_API int wcg_load_merged_device(wcg_ctx *ctx, const void *dev_bytes, uint64_t n, uint64_t *nlines);

/* The reference's JSON files into the aggregation tables, decoded on the device: lines
 * {"Key":"<key>","Value":"<value>"}\n as Go's json.Encoder writes them for letter-only keys.
 *   WCG_JSON_MAP  DoMap's intermediates mrtmp.<f>-<m>-<r> (mapreduce.go:214-230, what wcg_map_json
 *                 writes): every line is one occurrence of its key, its value is "1"
 *   WCG_JSON_RES  DoReduce's mrtmp.<f>-res-<r> (mapreduce.go:264-279, what wcg_partition* writes):
 *                 the line's value is its key's count
 * The file's keys are added to the context's tables as by wcg_map* / wcg_import: onto a live table
 * or after wcg_reset, counts adding as unsigned 64-bit; a full table is reported by the next
 * wcg_reduce / wcg_export_count.  *nlines = the lines imported.  Synchronous.  The host form copies
 * the file to a library-owned device buffer through the context's pinned staging buffers (as
 * wcg_load_merged) and then runs the device form's code.
 *   Parity.  MAP mode over the -<m>-<r> files of every map job m, then wcg_reduce and
 * wcg_partition(1, 0), gives the bytes DoReduce(r) writes (mapreduce.go:239-280).  RES mode over
 * every -res-<r>, then wcg_reduce, gives Merge's file (mapreduce.go:284-321) when the files' keys
 * are disjoint (a job's always are); a key present in several files adds, where Merge's map would
 * keep the last.
 *   n == 0: WCG_OK, nothing is touched.  A NULL pointer with n > 0, or another mode: WCG_EINVAL.
 * n > 0 with a last byte other than '\n': WCG_EINVAL ("newline" in wcg_last_error), checked first
 * (the host form: before the device is touched; the device form reads that one byte).
 *   The file is checked whole before anything is aggregated.  Per line (B = the line without its
 * '\n', L = its length), in this order:
 *   frame  L >= 10, B starts with {"Key":" and ends with "}
 *   value  V = the run of bytes other than '"' that ends at L-2, followed back for at most 21 bytes
 *          and never into B[0..8): V is not empty and a '"' opens it within those bounds; MAP: V is
 *          the single byte 1; RES: V is a canonical decimal in 1 .. 2^64-1 (first digit 1-9, at
 *          most 20 digits, no wrap)
 *   sep    the 11 bytes that end with V's opening quote are ","Value":" and begin at offset >= 8
 *   key    K = B[8 .. L-2-len(V)-11) has 1 .. 2^23-1 bytes and Go's tokenizer returns exactly K for
 *          K: every rune is valid UTF-8 and a unicode.IsLetter letter (so quotes, backslash
 *          escapes, digits, NUL and invalid UTF-8 all break it; letter-only keys never need JSON
 *          escaping, so the reference's decoder yields the same key bytes)
 * A file that breaks a rule: WCG_EINVAL, wcg_last_error() reads "wcg_import_json: line <N>: <rule>"
 * for the lowest offending line (N counts from 0) and the first rule it breaks; the context is
 * exactly as it was (tables, the last result and its caches, a pending wcg_reduce_async job).  An
 * accepted file drops results and pending jobs exactly as wcg_import does. */
enum { WCG_JSON_MAP = 0, WCG_JSON_RES = 1 };
WCG_API int wcg_import_json(wcg_ctx *ctx, const uint8_t *host_bytes, uint64_t n, int mode, uint64_t *nlines);
WCG_API int wcg_import_json_device(wcg_ctx *ctx, const void *dev_bytes, uint64_t n, int mode, uint64_t *nlines);

/* Per-phase device time of the last pipeline run, in milliseconds, measured with HIP events
 * on the context's stream: ms[0] map kernel (tokenize + LDS aggregation, summed over the
 * wcg_map* calls since wcg_reset), ms[1] long-token counting + miss-log aggregation kernels
 * (k_long_hash, k_long_agg, k_agg pass 1, k_rp, k_agg pass 2), ms[2] compaction,
 * ms[3] sort, ms[4] format; the shuffle of wcg_exchange: ms[5] export (counts + unit writes),
 * ms[6] RCCL exchange (counts all-to-all, its host read, grouped send/recv), ms[7] import;
 * wcg_gather_merge: ms[8] RCCL gather of the runs to root, ms[9] merge of the runs.
 * n = number of doubles the caller provides (<= 10). */
WCG_API int wcg_timings(wcg_ctx *ctx, double *ms, int n, uint64_t *map_launches);
/* Enable/disable the event timing above (off by default: it adds event records, each a ~5 us
 * bubble between the kernels it separates).  on = 1: the phases of the last job; on = 2: every job
 * from this call on, summed (wcg_reset keeps the events, so a timed loop needs no wcg_timings
 * call, and no host round trip, between its jobs); on = 3: as 2, the map kernel (ms[0]) only. */
WCG_API int wcg_enable_timing(wcg_ctx *ctx, int on);

/* Diagnostics, stats9 = {tokens, distinct keys, tokens counted in LDS, global-table operations,
 * tokens > 15 bytes, long-key heap bytes (keys > 32 bytes; shorter long keys live in their
 * table slot's cell), overflow, spin_fail, records emitted by the second aggregation pass}. */
WCG_API int wcg_stats(wcg_ctx *ctx, uint64_t *stats9);

/* Diagnostics: the last wcg_map_file / wcg_map ingest, from its own timers and events (ms unless
 * noted): out[0] host wall time until every chunk was issued, out[1] reading (pread + line scan)
 * on the calling thread and its reader pool, out[2] waiting for a free staging slot, out[3] the
 * chunks' H2D copies (sum of copy durations), out[4] the copy engine's span (first copy start to
 * last copy end), out[5] its idle fraction 1 - out[3] / out[4], out[6] the chunks' map kernels
 * (sum), out[7] device span from the first copy to the last chunk's map end, out[8] chunks.
 * Waits for the context's streams.  n = number of doubles the caller provides (<= 9). */
WCG_API int wcg_ingest_stats(wcg_ctx *ctx, double *out, int n);

/* Diagnostics: which reduce the last wcg_reduce ran: *path = 1 for the one-launch reduce of small
 * one-pass jobs (compaction, sort and formatting in one persistent kernel: jobs after the first of
 * a context whose previous job had at most 2^17 keys), 0 for the multi-launch path. */
WCG_API int wcg_reduce_path(const wcg_ctx *ctx, int *path);

/* Diagnostics: the seed of the map kernel's LDS key tables.  A context that has reduced a one-pass
 * job keeps that job's most frequent inline keys (<= 15 bytes) as a placed image, and its later
 * one-pass map calls start their LDS tables from it instead of empty: fewer tokens miss the
 * tables.  The seed is a hint like the record-count hint: it survives wcg_reset, and no result
 * depends on it.  A seeded job whose share of tokens counted in LDS falls below that of the
 * (unseeded) job the seed came from drops it; the next job runs unseeded and builds a new one.
 * WCG_SEED=0 in the environment switches seeding off.  stats3 = {the context holds a seed, seeds
 * built since wcg_open, the last finished job's map calls all ran seeded}. */
WCG_API int wcg_seed_stats(wcg_ctx *ctx, uint64_t *stats3);

/* FNV-1a 32 (= ihash, mapreduce.go:185-189), host side, for partition arithmetic. */
WCG_API uint32_t wcg_ihash(const uint8_t *key, uint64_t len);

WCG_API const char *wcg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WCG_H */
