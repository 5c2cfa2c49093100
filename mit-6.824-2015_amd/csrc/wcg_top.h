// wcg_top.h - the N highest-count words of the last reduce, selected on gfx950 (wcg_top).
//
// The reference's only acceptance check of word count is `sort -n -k2 mrtmp.kjv12.txt | tail -10`
// (src/main/test-wc.sh:2-3): the merged file's lines by count, the last ten.  After wcg_reduce the
// sorted records sit in HBM in exact bytewise key order, so that order is the total order
// (count as u64, index in the sorted records): no key byte is compared and the arena is not read.
//
//   k_top_select  TOP_NT-thread workgroups stride over tiles of TOP_TILE records (only each
//                 record's count word is loaded).  A workgroup keeps TOP_BUF candidate items in LDS
//                 and a threshold tau, the n-th largest item it has seen; a thread appends an item
//                 above tau through an LDS cursor.  When the buffer is full, the workgroup sorts it
//                 (bitonic, descending), keeps the first n, raises tau and takes the tile's items
//                 that found no room and still beat tau: a compaction per TOP_BUF - n appended items.
//                 Its <= n survivors go to a scratch array.
//   k_top_final   one workgroup runs the same selection over every workgroup's survivors (a second
//                 launch: the kernel boundary is the hand-over, no flag, fence or ticket) and writes
//                 the chosen records, ascending, for the formatter (wcg_reduce.h: k_fmt_*), with
//                 the number of lines and their exact byte size.
#pragma once
#include "wcg_common.h"
#include "wcg_reduce.h"

namespace wcg {

constexpr int TOP_NT = 256;          // threads per workgroup
constexpr int TOP_TILE = 1024;       // records per workgroup step
constexpr int TOP_BUF = 2048;        // candidate items in LDS (2 x u64 each: 32 KB)
constexpr int TOP_MAXG = 1024;       // largest grid of k_top_select (4 workgroups per CU)
constexpr int TOP_NMAX = 1024;       // largest n (WCG_TOP_MAX)
constexpr int TOP_FINAL = 262144;    // survivor slots (grid x n) the final stage reads at most
constexpr int TOP_IPT = TOP_TILE / TOP_NT;
// the scratch array: survivors per workgroup [TOP_MAXG], {lines, bytes}, then grid x n items
constexpr int TOP_HDR = TOP_MAXG + 2;
static_assert(TOP_TILE % TOP_NT == 0, "a thread takes TOP_IPT records of a tile");
static_assert(TOP_NMAX + TOP_TILE <= TOP_BUF, "after a compaction the buffer takes the rest of any tile");
static_assert((TOP_BUF & (TOP_BUF - 1)) == 0, "the bitonic sort pads to a power of two <= TOP_BUF");
static_assert(TOP_HDR % 2 == 0, "the items are stored 16 bytes at a time");
static_assert(TOP_FINAL / TOP_NMAX >= 1, "at least one workgroup at the largest n");

// item = (count, index in the sorted records), compared lexicographically; indices are distinct
__device__ __forceinline__ bool top_less(u64 ac, u64 ai, u64 bc, u64 bi) { return ac < bc || (ac == bc && ai < bi); }

struct TopLds {
    u64 cnt[TOP_BUF];
    u64 idx[TOP_BUF];
    u64 bytes;                       // k_top_final: the chosen lines' size
    u32 fill;                        // the append cursor
};

// Sort the m buffered items descending and keep the first min(m, n); when n were kept, (tc, ti)
// becomes the n-th largest.  Every thread calls it with the same m, behind a barrier after the
// last append; it ends with a barrier.  Returns the items kept.
__device__ __forceinline__ u32 top_compact(TopLds& s, u32 m, u32 n, u64& tc, u64& ti) {
    const u32 tid = threadIdx.x;
    u32 P = 2;
    while (P < m) P <<= 1;
    for (u32 i = m + tid; i < P; i += TOP_NT) { s.cnt[i] = 0; s.idx[i] = 0; }   // below every item
    __syncthreads();
    for (u32 k = 2; k <= P; k <<= 1)
        for (u32 j = k >> 1; j; j >>= 1) {
            for (u32 p = tid; p < P / 2; p += TOP_NT) {
                const u32 i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const u64 ac = s.cnt[i], ai = s.idx[i], bc = s.cnt[l], bi = s.idx[l];
                const bool desc = (i & k) == 0;
                if (top_less(ac, ai, bc, bi) == desc) {
                    s.cnt[i] = bc; s.idx[i] = bi;
                    s.cnt[l] = ac; s.idx[l] = ai;
                }
            }
            __syncthreads();
        }
    const u32 keep = m < n ? m : n;
    if (m >= n) { tc = s.cnt[n - 1]; ti = s.idx[n - 1]; }     // (appends land at keep and above)
    if (tid == 0) s.fill = keep;
    __syncthreads();
    return keep;
}

// The n largest of the `total` items of src, taking tiles first, first + stride, ...: sorted
// descending in s.cnt / s.idx[0, returned count).  src.load(i, c, x) gives item i, c = 0: none.
template <typename Src>
__device__ __forceinline__ u32 top_run(TopLds& s, const Src& src, u64 total, u32 n, u64 first, u64 stride) {
    const u32 tid = threadIdx.x;
    if (tid == 0) s.fill = 0;
    u64 tc = 0, ti = ~0ull;                        // tau: below every item with a count
    __syncthreads();
    const u64 ntiles = (total + TOP_TILE - 1) / TOP_TILE;
    u64 c[TOP_IPT], x[TOP_IPT];
#pragma unroll
    for (int k = 0; k < TOP_IPT; k++) {
        const u64 i = first * TOP_TILE + (u64)k * TOP_NT + tid;
        c[k] = 0; x[k] = 0;
        if (first < ntiles && i < total) src.load(i, c[k], x[k]);
    }
    for (u64 t = first; t < ntiles; t += stride) {
        // the next tile's loads are in flight across this tile's barriers
        u64 nc[TOP_IPT], nx[TOP_IPT];
        const u64 tn = t + stride;
#pragma unroll
        for (int k = 0; k < TOP_IPT; k++) {
            const u64 i = tn * TOP_TILE + (u64)k * TOP_NT + tid;
            nc[k] = 0; nx[k] = 0;
            if (tn < ntiles && i < total) src.load(i, nc[k], nx[k]);
        }
        // Append the items above tau; one that finds the buffer full stays with its thread, the
        // workgroup compacts, and what is still above the raised tau goes in behind the n kept
        // (n + TOP_TILE <= TOP_BUF: the second round always fits).
        u32 pend = 0;
#pragma unroll
        for (int k = 0; k < TOP_IPT; k++) pend |= (c[k] != 0 && top_less(tc, ti, c[k], x[k])) ? 1u << k : 0u;
        for (;;) {
#pragma unroll
            for (int k = 0; k < TOP_IPT; k++)
                if (pend >> k & 1) {
                    const u32 p = atomicAdd(&s.fill, 1u);
                    if (p < TOP_BUF) { s.cnt[p] = c[k]; s.idx[p] = x[k]; pend &= ~(1u << k); }
                }
            __syncthreads();
            const u32 m = s.fill;                   // workgroup-uniform: nothing appends before the next barrier
            if (m < TOP_BUF) { __syncthreads(); break; }
            (void)top_compact(s, TOP_BUF, n, tc, ti);            // full: TOP_BUF items are in it
            if (m == TOP_BUF) break;                             // and every item found its place
#pragma unroll
            for (int k = 0; k < TOP_IPT; k++)
                if ((pend >> k & 1) && !top_less(tc, ti, c[k], x[k])) pend &= ~(1u << k);
        }
#pragma unroll
        for (int k = 0; k < TOP_IPT; k++) { c[k] = nc[k]; x[k] = nx[k]; }
    }
    return top_compact(s, s.fill, n, tc, ti);
}

struct TopRecSrc {
    const Rec* r;
    __device__ __forceinline__ void load(u64 i, u64& c, u64& x) const { c = r[i].cnt; x = i; }
};

// the survivors of workgroup g: items [g * n, g * n + cand[g])
struct TopCandSrc {
    const u64* cand;
    u32 n;
    __device__ __forceinline__ void load(u64 i, u64& c, u64& x) const {
        const u64 g = i / n, j = i - g * n;
        if (j < cand[g]) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2*>(cand + TOP_HDR)[i];
            c = v.x; x = v.y;
        }
    }
};

// 1 <= n <= TOP_NMAX, gridDim.x <= TOP_MAXG; cand holds TOP_HDR + 2 * gridDim.x * n words
__global__ __launch_bounds__(TOP_NT) void k_top_select(const Rec* r, u64 nrec, u32 n, u64* cand) {
    __shared__ TopLds s;
    const u32 m = top_run(s, TopRecSrc{r}, nrec, n, blockIdx.x, gridDim.x);
    ulonglong2* const out = reinterpret_cast<ulonglong2*>(cand + TOP_HDR) + (u64)blockIdx.x * n;
    for (u32 j = threadIdx.x; j < m; j += TOP_NT) out[j] = make_ulonglong2(s.cnt[j], s.idx[j]);
    if (threadIdx.x == 0) cand[blockIdx.x] = m;
}

// One workgroup: the n largest of the grid x n survivor slots; out[0, q) (q = min(n, nrec)) gets
// their records in ascending (count, index) order, behind q - lines records of count 0 (which
// format to no line); cand[TOP_MAXG] = lines, cand[TOP_MAXG + 1] = bytes of "key: count\n".
__global__ __launch_bounds__(TOP_NT) void k_top_final(u64* cand, u32 grid, u32 n, const Rec* r, u32 q, Rec* out) {
    __shared__ TopLds s;
    if (threadIdx.x == 0) s.bytes = 0;
    const u32 m = top_run(s, TopCandSrc{cand, n}, (u64)grid * n, n, 0, 1);
    u64 b = 0;
    for (u32 j = threadIdx.x; j < q; j += TOP_NT) {
        Rec v;
        v.hi = v.lo = v.cnt = v.ref = 0;
        if (j < m) {
            v = r[s.idx[j]];
            b += line_len(v, FMT_MERGED, 1, 0, nullptr);
        }
        out[q - 1 - j] = v;
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(&s.bytes), b);
    __syncthreads();
    if (threadIdx.x == 0) { cand[TOP_MAXG] = m; cand[TOP_MAXG + 1] = s.bytes; }
}

}  // namespace wcg
