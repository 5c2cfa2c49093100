// wcg_bycount.h - the merged file in count order (wcg_by_count, wcg_count_rank), sorted on gfx950.
//
// `LC_ALL=C sort -n -k2 <merged file>` orders the lines by count (as u64) and lines of equal count
// by bytewise key.  After wcg_reduce the sorted records sit in HBM in exact bytewise key order, so
// that order is ascending (count, index in the sorted records): two integers per record, no key
// byte is compared and the arena is not read (wcg_top.h selects by the same order).
//
// The order is an LSD radix sort of the items (count u64, index u32) by the count's eight byte
// digits, least significant first, with a stable scatter per digit: the items start in index order
// and every pass keeps the order of equal digits, so equal counts end in index order and the index
// is never a sort key.  A digit in which all counts agree moves nothing and is skipped.
//
//   k_bc_items    reads the records once (the count word only), writes the items in index order and
//                 adds up the histograms of all eight digits and the number of zero counts (LDS
//                 histograms per workgroup, then integer atomics on 2049 global words: sums, so the
//                 order in which they land changes nothing).  The host reads those 16 KB once and
//                 decides the schedule: the digits with more than one non-empty bin.
//   per scheduled digit, three launches (each hand-over is a kernel boundary; no flag, ticket,
//   spin-wait or look-back between workgroups):
//   k_bc_count    workgroup g owns the tiles [g tpg, (g + 1) tpg) of BC_TILE items: its histogram of
//                 the digit, to hist[bin][g]
//   k_bc_scan     one workgroup: the exclusive prefix sums of hist in that (bin, g) order, which is
//                 where workgroup g's items with that digit start in the output
//   k_bc_scatter  workgroup g walks its tiles in order.  A wave owns 64 * BC_IPT consecutive items
//                 of a tile and takes them 64 at a time: eight __ballot rounds give each lane the
//                 64-bit mask of the lanes with its digit, popcount below the lane is its rank
//                 among them, and a per-wave LDS counter per bin carries the count over the wave's
//                 rounds.  A prefix over the tile's waves and the workgroup's running bases turn
//                 that into the output position: order (tile, wave, round, lane) = index order.
//   k_bc_gather   the records of a window of the order, into a scratch array for the formatter
//   k_bc_rank     a lower-bound binary search per query over the order's sorted count column
//
// Records of count 0 (the sort's merged duplicates: dd_same / long_same) sort to the front; their
// number z offsets every rank.
#pragma once
#include "wcg_common.h"

namespace wcg {

constexpr int BC_NT = 256;           // threads per workgroup
constexpr int BC_NW = BC_NT / 64;    // waves per workgroup
constexpr int BC_IPT = 8;            // items per thread and tile
constexpr int BC_TILE = 2048;        // items per tile
constexpr int BC_MAXG = 512;         // largest grid of the passes (2 workgroups per CU of 256)
constexpr int BC_BINS = 256;         // a digit is a byte
constexpr int BC_DIGITS = 8;
constexpr int BC_HIST = BC_DIGITS * BC_BINS + 1;   // k_bc_items' global words: the histograms, the zero counts
constexpr int BC_SCAN_NT = 1024;
static_assert(BC_TILE == BC_NT * BC_IPT, "a thread takes BC_IPT items of a tile");
static_assert(BC_NT == BC_BINS, "thread b owns bin b where a workgroup walks its bins");

// the mask of the wave's valid lanes whose digit equals this lane's (0 for a lane that is not
// valid).  Every lane of the wave calls it.
__device__ __forceinline__ u64 bc_match(u32 d, bool valid) {
    u64 m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1;
        const u64 v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return valid ? m : 0;
}

// Add the wave's digits to the LDS histogram h.  The lanes that share the first lane's digit go
// in as one add (most words occur a few times: the upper digits of a wave are all zero); the rest
// add one each.  Every lane calls it; an invalid lane passes d = 0, and the first lane is valid
// whenever any is (the lanes take ascending items).
__device__ __forceinline__ void bc_hist_add(u32* h, u32 d, bool valid, u32 lane) {
    const u32 first = __builtin_amdgcn_readfirstlane(d);
    const bool same = valid && d == first;
    const u64 m = __ballot(same);
    if (same) {
        if ((m & ((1ull << lane) - 1)) == 0) atomicAdd(&h[d], (u32)__popcll(m));
    } else if (valid) {
        atomicAdd(&h[d], 1u);
    }
}

// nrec < 2^32.  key[i] = r[i].cnt, idx[i] = i; hist[d * 256 + b] += the records whose digit d is b,
// hist[2048] += the records of count 0 (hist is zero at the launch)
__global__ __launch_bounds__(BC_NT) void k_bc_items(const Rec* __restrict__ r, u64 nrec, u64* __restrict__ key,
                                                    u32* __restrict__ idx, u64* __restrict__ hist) {
    __shared__ u32 h[BC_HIST];
    const u32 tid = threadIdx.x, lane = tid & 63;
    for (u32 j = tid; j < BC_HIST; j += BC_NT) h[j] = 0;
    __syncthreads();
    const u64 ntiles = (nrec + BC_TILE - 1) / BC_TILE;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u64 c[BC_IPT];
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const u64 i = t * BC_TILE + (u64)k * BC_NT + tid;
            c[k] = i < nrec ? r[i].cnt : 0;
        }
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const u64 i = t * BC_TILE + (u64)k * BC_NT + tid;
            const bool valid = i < nrec;
            if (valid) { key[i] = c[k]; idx[i] = (u32)i; }
#pragma unroll
            for (int d = 0; d < BC_DIGITS; d++) bc_hist_add(h + d * BC_BINS, (u32)(c[k] >> (8 * d)) & 255u, valid, lane);
            const u64 zero = __ballot(valid && c[k] == 0);
            if (lane == 0 && zero) atomicAdd(&h[BC_HIST - 1], (u32)__popcll(zero));
        }
    }
    __syncthreads();
    for (u32 j = tid; j < BC_HIST; j += BC_NT)
        if (h[j]) atomicAdd(reinterpret_cast<unsigned long long*>(&hist[j]), (unsigned long long)h[j]);
}

// item k of a thread in tile t: wave w owns the tile's items [w * 64 * BC_IPT, (w + 1) * 64 * BC_IPT)
__device__ __forceinline__ u64 bc_item(u64 t, u32 w, u32 lane, int k) {
    return t * BC_TILE + (u64)w * (64 * BC_IPT) + (u64)k * 64 + lane;
}

// gridDim.x = G workgroups, workgroup g owns the tiles [g * tpg, (g + 1) * tpg) of key[0, n):
// hist[b * G + g] = its items whose digit (key >> shift) & 255 is b
__global__ __launch_bounds__(BC_NT) void k_bc_count(const u64* __restrict__ key, u64 n, u32 shift, u32 tpg,
                                                    u32* __restrict__ hist) {
    __shared__ u32 h[BC_BINS];
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    h[tid] = 0;
    __syncthreads();
    const u64 ntiles = (n + BC_TILE - 1) / BC_TILE;
    const u64 t0 = (u64)blockIdx.x * tpg, t1 = t0 + tpg < ntiles ? t0 + tpg : ntiles;
    for (u64 t = t0; t < t1; t++) {
        u64 c[BC_IPT];
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const u64 i = bc_item(t, w, lane, k);
            c[k] = i < n ? key[i] : 0;
        }
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const bool valid = bc_item(t, w, lane, k) < n;
            bc_hist_add(h, valid ? (u32)(c[k] >> shift) & 255u : 0u, valid, lane);
        }
    }
    __syncthreads();
    hist[(u64)tid * gridDim.x + blockIdx.x] = h[tid];
}

// one workgroup: h[0, n) becomes its exclusive prefix sums (n <= 256 * BC_MAXG; the total is the
// item count, below 2^32)
__global__ __launch_bounds__(BC_SCAN_NT) void k_bc_scan(u32* __restrict__ h, u32 n) {
    __shared__ u32 s[BC_SCAN_NT];
    const u32 tid = threadIdx.x;
    const u32 per = (n + BC_SCAN_NT - 1) / BC_SCAN_NT;
    const u32 a = tid * per < n ? tid * per : n, b = a + per < n ? a + per : n;
    u32 sum = 0;
    for (u32 i = a; i < b; i++) sum += h[i];
    s[tid] = sum;
    __syncthreads();
    for (u32 o = 1; o < BC_SCAN_NT; o <<= 1) {
        const u32 v = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    u32 run = s[tid] - sum;
    for (u32 i = a; i < b; i++) {
        const u32 v = h[i];
        h[i] = run;
        run += v;
    }
}

// The stable scatter of one digit: grid and tpg as k_bc_count's, hist = its scanned histogram.
// Items with equal digits keep their order; kout / xout are other buffers than kin / xin.
__global__ __launch_bounds__(BC_NT) void k_bc_scatter(const u64* __restrict__ kin, const u32* __restrict__ xin, u64 n,
                                                      u32 shift, u32 tpg, const u32* __restrict__ hist,
                                                      u64* __restrict__ kout, u32* __restrict__ xout) {
    __shared__ u32 wc[BC_NW][BC_BINS];     // per wave: the items of each bin in its rounds so far
    __shared__ u32 off[BC_NW][BC_BINS];    // per wave: where its items of each bin start in the output
    __shared__ u32 base[BC_BINS];          // where the workgroup's next item of each bin goes
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 below = (1ull << lane) - 1;
    base[tid] = hist[(u64)tid * gridDim.x + blockIdx.x];
#pragma unroll
    for (int v = 0; v < BC_NW; v++) wc[v][tid] = 0;
    __syncthreads();
    const u64 ntiles = (n + BC_TILE - 1) / BC_TILE;
    const u64 t0 = (u64)blockIdx.x * tpg, t1 = t0 + tpg < ntiles ? t0 + tpg : ntiles;
    for (u64 t = t0; t < t1; t++) {
        u64 c[BC_IPT];
        u32 x[BC_IPT], lr[BC_IPT];
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const u64 i = bc_item(t, w, lane, k);
            c[k] = 0; x[k] = 0;
            if (i < n) { c[k] = kin[i]; x[k] = xin[i]; }
        }
        // the rank of every item among its wave's items of the same bin, in (round, lane) order.
        // The barriers keep a round's reads of the counters before its leader's write and that
        // write before the next round's reads (every thread runs every round).
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            const bool valid = bc_item(t, w, lane, k) < n;
            const u32 d = (u32)(c[k] >> shift) & 255u;
            const u64 m = bc_match(d, valid);
            const u32 r = (u32)__popcll(m & below);
            const u32 pre = valid ? wc[w][d] : 0;
            lr[k] = pre + r;
            __syncthreads();
            if (valid && r == 0) wc[w][d] = pre + (u32)__popcll(m);
            __syncthreads();
        }
        // bin tid: the waves' counts to their starts behind the workgroup's base; the counters are
        // cleared for the next tile
        {
            u32 run = base[tid];
#pragma unroll
            for (int v = 0; v < BC_NW; v++) {
                const u32 cnt = wc[v][tid];
                off[v][tid] = run;
                wc[v][tid] = 0;
                run += cnt;
            }
            base[tid] = run;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BC_IPT; k++) {
            if (bc_item(t, w, lane, k) >= n) continue;
            const u64 dst = (u64)off[w][(u32)(c[k] >> shift) & 255u] + lr[k];
            if (dst < n) { kout[dst] = c[k]; xout[dst] = x[k]; }     // (always: hist counted these items)
        }
        // off is written again behind the next tile's round barriers
    }
}

// out[j] = r[idx[pos + j]], j < m: the records at positions [pos, pos + m) of the order (an index
// that names no record gives a record without a count, which the caller's line count shows)
__global__ __launch_bounds__(BC_NT) void k_bc_gather(const Rec* __restrict__ r, u64 nrec, const u32* __restrict__ idx, u64 pos,
                                                     u64 m, Rec* __restrict__ out) {
    for (u64 j = (u64)blockIdx.x * BC_NT + threadIdx.x; j < m; j += (u64)gridDim.x * BC_NT) {
        const u32 x = idx[pos + j];
        ulonglong2 a = make_ulonglong2(0, 0), b = a;
        if (x < nrec) {
            a = *reinterpret_cast<const ulonglong2*>(&r[x].hi);
            b = *reinterpret_cast<const ulonglong2*>(&r[x].cnt);
        }
        *reinterpret_cast<ulonglong2*>(&out[j].hi) = a;
        *reinterpret_cast<ulonglong2*>(&out[j].cnt) = b;
    }
}

// out[i] = the keys whose count is below q[i]: the lower bound of q[i] in the ascending key[0, n),
// less the z zero counts at its front (which no query exceeds unless it is above zero)
__global__ __launch_bounds__(BC_NT) void k_bc_rank(const u64* __restrict__ key, u64 n, u64 z, const u64* __restrict__ q,
                                                   u64 nq, u64* __restrict__ out) {
    for (u64 i = (u64)blockIdx.x * BC_NT + threadIdx.x; i < nq; i += (u64)gridDim.x * BC_NT) {
        const u64 v = q[i];
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (key[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        out[i] = lo > z ? lo - z : 0;
    }
}

}  // namespace wcg
