// wcg_query.h - point queries and key ranges over the last reduce's sorted records (wcg_lookup,
// wcg_range), on gfx950.
//
// After wcg_reduce the records sit in HBM in exact bytewise key order (wcg_sort.h), so "how often
// does this word occur" and "the lines from A to B" are binary searches over them; only the
// answer crosses to the host.
//
//   rec_cmp       THE comparator: a record against (query bytes, length), three-way, in the full
//                 bytewise order of the merged file.  Everything below decides through it.
//   k_lookup      LK_NT-thread workgroups stride over tiles of LK_TILE queries; a thread runs LK_Q
//                 lower-bound searches interleaved, so that LK_Q dependent loads are in flight per
//                 lane (a search is a chain of L2 hits and HBM misses, nothing else).
//                 MODE LK_COUNT writes the found record's count (0: the key does not occur),
//                 MODE LK_INDEX the lower bound itself (wcg_range's two bounds).
//                 LDS: the workgroup first stages the hi word of LK_S evenly spaced records in
//                 LDS and narrows every search there (the top 11 steps are LDS reads, not L2
//                 hits); it costs LK_S strided loads per workgroup, so only batches of
//                 LK_LDS_MIN queries and more take it (DESIGN.md section 20 has both timings).
//   k_range_size  the lines of records [a, b) and their exact byte size, per workgroup;
//   k_range_total one workgroup adds those up (a second launch: the kernel boundary is the
//                 hand-over, no atomic on global memory).
#pragma once
#include "wcg_common.h"
#include "wcg_reduce.h"

namespace wcg {

constexpr int LK_NT = 256;           // threads per workgroup
constexpr int LK_Q = 4;              // searches a thread runs interleaved
constexpr int LK_TILE = 1024;        // queries per workgroup step
constexpr int LK_MAXG = 2048;        // largest grid of k_lookup (8 workgroups per CU of 256: every CU stays fed)
constexpr int RS_NT = 256;
constexpr int RS_MAXG = 1024;        // largest grid of k_range_size
constexpr int LK_COUNT = 0, LK_INDEX = 1;
constexpr int LK_S = 2048;           // splitters a workgroup of the LDS variant stages (16 KB)
constexpr int LK_LDS_MIN = 524288;   // queries from which a batch takes the LDS variant (two tiles per CU of 256)
static_assert((LK_S & (LK_S - 1)) == 0, "the splitter search halves a power of two");
static_assert(LK_TILE == LK_NT * LK_Q, "query k of a thread is tile * LK_TILE + k * LK_NT + tid: coalesced writes");

// the 16-byte big-endian prefix of a query, zero-padded (what a record's hi, lo are of its key)
__device__ __forceinline__ void query_prefix(const uint8_t* q, u64 len, u64& qh, u64& ql) {
    qh = ql = 0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
        const u64 v = (u64)b < len ? q[b] : 0;
        if (b < 8) qh |= v << (56 - 8 * b);
        else ql |= v << (120 - 8 * b);
    }
}

// Record (prefix hi, lo; ref) against the query (bytes q[0, len), prefix qh, ql): < 0, 0, > 0 as
// the record's key sorts before, equals or sorts after the query, bytewise, a prefix first.
//   Unequal prefixes decide: a record key holds no zero byte (fact F4), so where the record's
//   padding meets a query byte the record is the shorter string and its 0 is the smaller byte,
//   and where the query's padding meets a record byte it is the other way round; a zero byte
//   inside the query is below every record byte, as it should be.
//   Equal prefixes, inline record (length ref < 16): the record's bytes are the query's first ref
//   bytes, and the query is not shorter (a shorter query would pad against a non-zero record
//   byte), so the lengths decide: "ab" sorts before the query "ab\0" and equals only "ab".
//   Equal prefixes, long record: the query has 16 non-zero bytes too; bytes from 16 on decide,
//   then the lengths.
__device__ __forceinline__ int rec_cmp(u64 hi, u64 lo, u64 ref, const uint8_t* arena, const uint8_t* q, u64 len,
                                       u64 qh, u64 ql) {
    if (hi != qh) return hi < qh ? -1 : 1;
    if (lo != ql) return lo < ql ? -1 : 1;
    Rec x;
    x.hi = hi; x.lo = lo; x.cnt = 0; x.ref = ref;
    const u64 rl = rec_len(x);
    if (ref & LONG_FLAG) {
        const u64 m = rl < len ? rl : len;
        for (u64 k = 16; k < m; k++) {
            const u32 a = rec_byte(x, k, arena), b = q[k];
            if (a != b) return a < b ? -1 : 1;
        }
    }
    return rl < len ? -1 : (rl > len ? 1 : 0);
}

// the record of splitter j < LK_S: non-decreasing in j and below nrec (nrec < 2^40: no overflow)
__device__ __forceinline__ u64 lk_pos(u64 j, u64 nrec) { return (j + 1) * nrec / (LK_S + 1); }

// nrec >= 1.  keys / off as wcg_lookup's (off has nq + 1 entries); out has nq entries.
template <int MODE, bool LDS>
__global__ __launch_bounds__(LK_NT) void k_lookup(const Rec* __restrict__ r, u64 nrec, const uint8_t* __restrict__ arena,
                                                  const uint8_t* __restrict__ keys, const u64* __restrict__ off, u64 nq,
                                                  u64* __restrict__ out) {
    const u64 ntiles = (nq + LK_TILE - 1) / LK_TILE;
    __shared__ u64 S[LDS ? LK_S : 1];
    if (LDS) {
        for (u32 j = threadIdx.x; j < LK_S; j += LK_NT) S[j] = r[lk_pos(j, nrec)].hi;
        __syncthreads();
    }
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 q0 = t * LK_TILE + threadIdx.x;
        const uint8_t* q[LK_Q];
        u64 len[LK_Q], qh[LK_Q], ql[LK_Q], lo[LK_Q], hi[LK_Q];
#pragma unroll
        for (int k = 0; k < LK_Q; k++) {
            const u64 i = q0 + (u64)k * LK_NT;
            const bool live = i < nq;
            const u64 o = live ? off[i] : 0, e = live ? off[i + 1] : 0;
            q[k] = keys + o;
            len[k] = e - o;
            query_prefix(q[k], len[k], qh[k], ql[k]);
            lo[k] = 0;
            hi[k] = live ? nrec : 0;               // a query past the batch searches nothing
        }
        if (LDS) {
            // a = the splitters whose hi is below the query's: their records, and all before
            // them, are below the query, so the lower bound lies behind splitter a - 1's record;
            // b = the first splitter whose hi is above the query's: its record is above the
            // query, so the lower bound is at most its index.  (Splitters with an equal hi say
            // nothing: lo and the rest of the key decide.)  S[a - 1] < S[b], so lo <= hi.
            u32 a[LK_Q], b[LK_Q];
#pragma unroll
            for (int k = 0; k < LK_Q; k++) a[k] = b[k] = 0;
            for (u32 s = LK_S / 2; s; s >>= 1) {
#pragma unroll
                for (int k = 0; k < LK_Q; k++) {
                    a[k] += S[a[k] + s - 1] < qh[k] ? s : 0;
                    b[k] += S[b[k] + s - 1] <= qh[k] ? s : 0;
                }
            }
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                a[k] += S[a[k]] < qh[k] ? 1 : 0;
                b[k] += S[b[k]] <= qh[k] ? 1 : 0;
                if (hi[k]) {
                    if (a[k]) lo[k] = lk_pos(a[k] - 1, nrec) + 1;
                    if (b[k] < LK_S) hi[k] = lk_pos(b[k], nrec);
                }
            }
        }
        // lower bound: the first record not below the query.  Every round loads the LK_Q middle
        // prefixes (one 16-byte load each, issued back to back; a finished search re-reads a
        // record it has seen) and only then compares.
        for (;;) {
            bool any = false;
#pragma unroll
            for (int k = 0; k < LK_Q; k++) any |= lo[k] < hi[k];
            if (!any) break;
            u64 mid[LK_Q];
            ulonglong2 p[LK_Q];
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                mid[k] = lo[k] + ((hi[k] - lo[k]) >> 1);
                p[k] = *reinterpret_cast<const ulonglong2*>(&r[mid[k] < nrec ? mid[k] : nrec - 1].hi);
            }
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                if (lo[k] >= hi[k]) continue;
                int c;
                if (p[k].x != qh[k] || p[k].y != ql[k]) c = (p[k].x < qh[k] || (p[k].x == qh[k] && p[k].y < ql[k])) ? -1 : 1;
                else c = rec_cmp(p[k].x, p[k].y, r[mid[k]].ref, arena, q[k], len[k], qh[k], ql[k]);
                if (c < 0) lo[k] = mid[k] + 1;
                else hi[k] = mid[k];
            }
        }
        if (MODE == LK_INDEX) {
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                const u64 i = q0 + (u64)k * LK_NT;
                if (i < nq) out[i] = lo[k];
            }
        } else {
            // Repeated keys are adjacent and the first record of a run carries the run's total
            // (wcg_sort.h: dd_same, k_tie_sort), so the lower bound is the record to read; a
            // record of count 0 without an equal predecessor is a key that does not occur.
            ulonglong2 p[LK_Q], c[LK_Q];
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                const Rec* const x = &r[lo[k] < nrec ? lo[k] : nrec - 1];
                p[k] = *reinterpret_cast<const ulonglong2*>(&x->hi);
                c[k] = *reinterpret_cast<const ulonglong2*>(&x->cnt);
            }
#pragma unroll
            for (int k = 0; k < LK_Q; k++) {
                const u64 i = q0 + (u64)k * LK_NT;
                if (i >= nq) continue;
                const bool eq = lo[k] < nrec && rec_cmp(p[k].x, p[k].y, c[k].y, arena, q[k], len[k], qh[k], ql[k]) == 0;
                out[i] = eq ? c[k].x : 0;
            }
        }
    }
}

// records [a, b) of r, b - a >= 1: part[2 g], part[2 g + 1] = the lines (records with a count)
// and the bytes of "key: count\n" that workgroup g saw
__global__ __launch_bounds__(RS_NT) void k_range_size(const Rec* __restrict__ r, u64 a, u64 b, u64* __restrict__ part) {
    __shared__ u64 ws[2][RS_NT / 64];
    u64 lines = 0, bytes = 0;
    for (u64 i = a + (u64)blockIdx.x * RS_NT + threadIdx.x; i < b; i += (u64)gridDim.x * RS_NT) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(&r[i].cnt);
        Rec x;
        x.hi = x.lo = 0; x.cnt = v.x; x.ref = v.y;
        lines += v.x != 0;
        bytes += line_len(x, FMT_MERGED, 1, 0, nullptr);
    }
    for (int d = 32; d; d >>= 1) { lines += __shfl_down(lines, d, 64); bytes += __shfl_down(bytes, d, 64); }
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = lines; ws[1][threadIdx.x >> 6] = bytes; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lines = bytes = 0;
        for (int w = 0; w < RS_NT / 64; w++) { lines += ws[0][w]; bytes += ws[1][w]; }
        part[2 * blockIdx.x] = lines;
        part[2 * blockIdx.x + 1] = bytes;
    }
}

// one workgroup: tot[0], tot[1] = the sums over the grid's parts
__global__ __launch_bounds__(RS_NT) void k_range_total(const u64* __restrict__ part, u32 grid, u64* __restrict__ tot) {
    __shared__ u64 ws[2][RS_NT / 64];
    u64 lines = 0, bytes = 0;
    for (u32 g = threadIdx.x; g < grid; g += RS_NT) { lines += part[2 * g]; bytes += part[2 * g + 1]; }
    for (int d = 32; d; d >>= 1) { lines += __shfl_down(lines, d, 64); bytes += __shfl_down(bytes, d, 64); }
    if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = lines; ws[1][threadIdx.x >> 6] = bytes; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lines = bytes = 0;
        for (int w = 0; w < RS_NT / 64; w++) { lines += ws[0][w]; bytes += ws[1][w]; }
        tot[0] = lines;
        tot[1] = bytes;
    }
}

}  // namespace wcg
