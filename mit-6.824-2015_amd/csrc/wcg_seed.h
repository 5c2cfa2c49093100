// wcg_seed.h - the seed image of k_map's LDS key tables, built from a reduce's sorted records.
//
// k_map's tables start empty, fill with whatever recurs first and never evict: on the C2 corpus a
// quarter of the tokens miss them.  A context that has reduced one job knows
// which keys are frequent, and the next job of a MapReduce worker is another split of the same
// corpus.  The seed image is a placed copy of the key words of k_map's tables - sk0[MAP_NS] |
// mk0[MAP_NM] | mk1[MAP_NM], counts implied zero - that k_map<MAP_SEEDED, true> copies into LDS
// instead of zeroing them.  A seeded slot is an ordinary slot with count 0: its key's first
// occurrence is a hit, and the flush skips it when the key never occurs.  The result of a job
// never depends on the image (any placed identities give exact counts); only the hit rate does.
//
// The image holds the highest-count inline keys of the records: up to SEED_FRAC of the slots of
// each kind (short <= 7 bytes, medium 8-15 bytes; long keys take no part).  Selection needs no
// sort: a histogram of floor(log2 count) per kind gives the threshold bin, every key above it is
// taken and the threshold bin's keys are admitted through a counter until the target is reached.
// Placement is by the kernel's own MapTable::slots() and key identity, first choice then second,
// by CAS; a key that finds both taken is dropped.  Bins are placed from the highest down (one
// workgroup, the image in LDS, a barrier between bins), so a frequent key never loses its slots
// to a rarer one: a seed never leaves, and a hot key shut out by it would miss for the whole job.
//
// Three launches behind a reduce, no host round trip; they run only when the context has no
// valid seed (wcg_api.hip), so a steady stream of jobs pays nothing for them.
#pragma once
#include "wcg_common.h"
#include "wcg_lds_table.h"
#include "wcg_map.h"

namespace wcg {

// share of each table's slots offered to seed keys (tools/hit_sim.py: 0.5 / 0.75 / 0.9 / 1.0 give
// 0.770 / 0.779 / 0.781 / 0.783 on C2, while a seed of keys that never occur costs 0.555 / 0.415 /
// 0.33 against 0.734 unseeded: the last quarter buys half a point and doubles a stale seed's cost)
constexpr u32 SEED_NUM = 3, SEED_DEN = 4;
constexpr u32 SEED_TS = (u32)MAP_NS * SEED_NUM / SEED_DEN;     // short keys offered
constexpr u32 SEED_TM = (u32)MAP_NM * SEED_NUM / SEED_DEN;     // medium keys offered
constexpr u32 SEED_NCAND = SEED_TS + SEED_TM;
constexpr u32 SEED_BINS = 64;                                  // floor(log2 count) of a u64 count
constexpr u64 SEED_IMG_WORDS = (u64)MAP_NS + 2ull * MAP_NM;     // sk0 | mk0 | mk1
static_assert(MAP_NS % 2 == 0 && MAP_NM % 2 == 0, "the image is copied 16 bytes at a time");

// the builder's scratch, after the image in one allocation
struct SeedScratch {
    u32 hist[2][SEED_BINS];          // keys per (kind, bin); kind 0 = short, 1 = medium
    u32 ctr[2][2];                   // per kind: candidates taken above the threshold bin, in it
    u64 job[2];                      // {tokens, lds_hits} of the job the image was built from: the
                                     // host compares later jobs with it, and may never have read
                                     // that job back (wcg_reduce_async dropped by the next map call)
    u32 bin[SEED_NCAND];             // candidates: short ones in [0, SEED_TS), medium ones after
    u64 k0[SEED_NCAND];
    u64 k1[SEED_NCAND];
};
constexpr u64 SEED_ZERO_BYTES = sizeof(u32) * (2 * SEED_BINS + 4);   // hist and ctr, zeroed per build
constexpr u64 SEED_ALLOC_BYTES = SEED_IMG_WORDS * sizeof(u64) + sizeof(SeedScratch);

constexpr int SEED_NT = 256;         // k_seed_hist, k_seed_pick
constexpr int SEED_PLACE_NT = 1024;  // k_seed_place: one workgroup
constexpr u32 SEED_CPT = (SEED_NCAND + SEED_PLACE_NT - 1) / SEED_PLACE_NT;   // candidates per thread

// records [0, n): n = min(*dev_n, ncap) when the count is still on the device (the fused reduce)
__device__ __forceinline__ u64 seed_nrec(u64 ncap, const u64* dev_n) {
    if (!dev_n) return ncap;
    const u64 n = *dev_n;
    return n < ncap ? n : ncap;
}

// an inline record's kind and bin from its {cnt, ref} half; false for long keys and empty counts
__device__ __forceinline__ bool seed_kind_bin(u64 cnt, u64 ref, u32& kind, u32& bin) {
    if (ref == 0 || ref > 15 || cnt == 0) return false;
    kind = ref >= 8 ? 1u : 0u;
    bin = 63u - (u32)__builtin_clzll(cnt);
    return true;
}

// the threshold of one kind: every key in a bin above T is taken (`above` of them, < target), and
// `take` keys of bin T.  Fewer keys than the target: T = 0 and every key is taken.
__device__ __forceinline__ void seed_threshold(const u32* hist, u32 target, u32& T, u32& above, u32& take) {
    u32 acc = 0;
    for (int b = SEED_BINS - 1; b >= 0; b--) {
        const u32 hb = hist[b];
        if (acc + hb >= target || b == 0) {
            T = (u32)b;
            above = acc;
            take = hb < target - acc ? hb : target - acc;
            return;
        }
        acc += hb;
    }
}

// positions for the lanes that want one: one atomic per wave
__device__ __forceinline__ u32 seed_reserve(u32* ctr, bool want) {
    const u64 m = __ballot(want);
    if (m == 0) return 0;
    const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
    const int leader = __builtin_ctzll(m);
    u32 base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(ctr, (u32)__popcll(m));
    return (u32)__shfl((int)base, leader, 64) + rank;
}

__global__ __launch_bounds__(SEED_NT) void k_seed_hist(const Rec* rec, u64 ncap, const u64* dev_n, SeedScratch* sc) {
    __shared__ u32 lh[2 * SEED_BINS];
    for (int i = threadIdx.x; i < 2 * (int)SEED_BINS; i += SEED_NT) lh[i] = 0;
    __syncthreads();
    const u64 n = seed_nrec(ncap, dev_n);
    for (u64 i = (u64)blockIdx.x * SEED_NT + threadIdx.x; i < n; i += (u64)gridDim.x * SEED_NT) {
        const ulonglong2 cr = *reinterpret_cast<const ulonglong2*>(&rec[i].cnt);   // {cnt, ref}
        u32 kind, bin;
        if (seed_kind_bin(cr.x, cr.y, kind, bin)) atomicAdd(&lh[kind * SEED_BINS + bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * (int)SEED_BINS; i += SEED_NT)
        if (lh[i]) atomicAdd(&sc->hist[0][0] + i, lh[i]);
}

__global__ __launch_bounds__(SEED_NT) void k_seed_pick(const Rec* rec, u64 ncap, const u64* dev_n, SeedScratch* sc) {
    __shared__ u32 sT[2], sAbove[2], sTake[2];
    if (threadIdx.x < 2)
        seed_threshold(sc->hist[threadIdx.x], threadIdx.x ? SEED_TM : SEED_TS, sT[threadIdx.x], sAbove[threadIdx.x],
                       sTake[threadIdx.x]);
    __syncthreads();
    const u64 n = seed_nrec(ncap, dev_n);
    // whole waves walk the records together (seed_reserve's ballot)
    for (u64 base = (u64)blockIdx.x * SEED_NT; base < n; base += (u64)gridDim.x * SEED_NT) {
        const u64 i = base + threadIdx.x;
        Rec r{0, 0, 0, 0};
        if (i < n) r = rec[i];
        u32 kind = 0, bin = 0;
        const bool ok = seed_kind_bin(r.cnt, r.ref, kind, bin);
#pragma unroll
        for (u32 kd = 0; kd < 2; kd++) {
            const bool mine = ok && kind == kd;
            const bool hi = mine && bin > sT[kd], at = mine && bin == sT[kd];
            const u32 ph = seed_reserve(&sc->ctr[kd][0], hi);
            const u32 pa = seed_reserve(&sc->ctr[kd][1], at);
            const u32 target = kd ? SEED_TM : SEED_TS;
            u32 pos = target;
            if (hi) pos = ph;
            if (at && pa < sTake[kd]) pos = sAbove[kd] + pa;
            if (pos < target) {
                const u32 q = (kd ? SEED_TS : 0u) + pos;
                u64 k0, k1;
                rec_inline_key(r, k0, k1);
                sc->k0[q] = k0; sc->k1[q] = k1; sc->bin[q] = bin;
            }
        }
    }
}

__global__ __launch_bounds__(SEED_PLACE_NT) void k_seed_place(SeedScratch* sc, u64* img, const DevState* st) {
    __shared__ __align__(16) u64 sk0[MAP_NS];
    __shared__ __align__(16) u64 mk0[MAP_NM];
    __shared__ __align__(16) u64 mk1[MAP_NM];
    __shared__ u32 sN[2], sLo, sHi;
    const int tid = threadIdx.x;
    for (int i = tid; i < MAP_NS; i += SEED_PLACE_NT) sk0[i] = 0;
    for (int i = tid; i < MAP_NM; i += SEED_PLACE_NT) { mk0[i] = 0; mk1[i] = 0; }
    if (tid < 2) {
        u32 T, above, take;
        seed_threshold(sc->hist[tid], tid ? SEED_TM : SEED_TS, T, above, take);
        sN[tid] = above + take;                    // candidates written by k_seed_pick
    }
    if (tid == 0) {                                // the bins that hold any key
        sc->job[0] = st->tokens;
        sc->job[1] = st->lds_hits;
        u32 lo = SEED_BINS, hi = 0;
        for (u32 b = 0; b < SEED_BINS; b++)
            if (sc->hist[0][b] | sc->hist[1][b]) { if (lo == SEED_BINS) lo = b; hi = b; }
        sLo = lo; sHi = hi;
    }
    __syncthreads();
    u64 k0[SEED_CPT], k1[SEED_CPT];
    u32 bin[SEED_CPT];                             // SEED_BINS: no candidate
#pragma unroll
    for (u32 j = 0; j < SEED_CPT; j++) {
        const u32 q = j * SEED_PLACE_NT + tid;
        const bool live = q < SEED_TS ? q < sN[0] : (q < SEED_NCAND && q - SEED_TS < sN[1]);
        k0[j] = live ? sc->k0[q] : 0;
        k1[j] = live ? sc->k1[q] : 0;
        bin[j] = live ? sc->bin[q] : SEED_BINS;
    }
    using Tab = MapTable<MAP_NS, MAP_NM>;
    if (sLo < SEED_BINS)
    for (int b = (int)sHi; b >= (int)sLo; b--) {   // workgroup-uniform
#pragma unroll
        for (u32 j = 0; j < SEED_CPT; j++) {
            if (bin[j] != (u32)b) continue;
            const bool med = !key_short(k0[j]);
            const u32 h = lds_hash(k0[j], k1[j]);
            u32 s1, s2;
            Tab::slots(h, med ? (u32)MAP_NM : (u32)MAP_NS, s1, s2);
            u64* const K0 = med ? mk0 : sk0;
            u32 s = s1;
            u64 old = atomicCAS(&K0[s], 0ull, k0[j]);
            if (old != 0) { s = s2; old = atomicCAS(&K0[s], 0ull, k0[j]); }
            if (old == 0 && med) mk1[s] = k1[j];
        }
        __syncthreads();
    }
    for (int i = tid; i < MAP_NS; i += SEED_PLACE_NT) img[i] = sk0[i];
    for (int i = tid; i < MAP_NM; i += SEED_PLACE_NT) { img[MAP_NS + i] = mk0[i]; img[MAP_NS + MAP_NM + i] = mk1[i]; }
}

}  // namespace wcg
