// wcg_index.h - query records of a merged file (wcg_index_merged), on gfx950.
//
// wcg_merge_runs leaves L sorted line records {hi, lo = the key's first 16 bytes, cnt = line
// bytes, ref = LONG_FLAG? | key length << 40 | offset in the merge's INPUT} (k_line_recs,
// wcg_reduce.h) and the lines themselves, in record order, in the context's result buffer.  The
// query kernels (wcg_top.h, wcg_query.h) want {hi, lo, cnt = the count, ref = key length, or
// LONG_FLAG | key length << 40 | offset of the key in an arena}.  The result buffer is that arena:
// line i starts at the exclusive sum of the line lengths before it, so no byte of the merge's
// input (the caller's memory) is read again.
//
//   k_ix_sum    bytes of each tile of FM_TILE = 1024 lines (k_scan_u64 turns them into offsets)
//   k_ix_write  per tile: the line offsets (a scan inside the tile), the tile's text staged in
//               LDS by aligned 16-byte loads (a tile past IX stage bytes - long keys - is read
//               in place), every count parsed backwards from its '\n', every rule of a merged
//               file checked, the query records written.
//
// The rules (wcg.check_merged states them on the host), per line, in this order:
//   count  the line is key, ": ", a canonical decimal in 1 .. 2^64-1 (first digit 1-9, at most 20
//          digits), '\n', and the ": " starts exactly where k_line_recs ended the key (the first ':')
//   zero   the count is not "0" (a record of count 0 means "merged duplicate, no line" downstream)
//   nul    the key holds no zero byte (rec_cmp's fact F4: prefixes pad with zeros)
//   order  the key sorts strictly after the previous line's, bytewise, a prefix first
// A broken rule is reported, never a fault: err[kind] = the lowest offending line (atomicMin, which
// only the error path touches); the host takes the lowest line, and the first kind above on a tie.
//
// Bounds.  Every text read lies inside the tile's span [t0, t0 + all) or, for the previous line of
// the tile's first record, inside that line's bytes just before t0; a tile whose span would pass
// the text's end (impossible for records k_line_recs made: their lengths sum to the text's size)
// reads nothing.  The backward parse of a count stops at the line's first byte; the position of
// ": " is not searched for but computed from the lengths, and looked at only when
// line bytes == key bytes + 2 + digits + 1, which puts it inside the line.
#pragma once
#include "wcg_common.h"
#include "wcg_reduce.h"

namespace wcg {

constexpr int IX_COUNT = 0, IX_ZERO = 1, IX_NUL = 2, IX_ORDER = 3, IX_KINDS = 4;
constexpr u64 IX_NONE = ~0ull;
constexpr u64 IX_U64_DIV10 = 1844674407370955161ull;   // (2^64 - 1) / 10; the last digit is then at most 5

__global__ __launch_bounds__(FM_NT) void k_ix_sum(const Rec* __restrict__ r, u64 n, u64* __restrict__ tsum) {
    __shared__ u64 ws[FM_NT / 64];
    const u64 i0 = (u64)blockIdx.x * FM_TILE + (u64)threadIdx.x * FM_IPT;
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < FM_IPT; k++) s += i0 + k < n ? r[i0 + k].cnt : 0;
    u64 all;
    (void)block_excl_scan(s, ws, all);
    if (threadIdx.x == 0) tsum[blockIdx.x] = all;
}

// the text: g[p] for any p; a staged tile also has sb[p - base] == g[p] for t0 <= p < t1
struct IxText {
    const uint8_t* g;
    const uint8_t* sb;
    u64 base, t0, t1;
};
template <bool STAGED>
__device__ __forceinline__ u32 ix_byte(const IxText& t, u64 p) {
    if (STAGED && p >= t.t0 && p < t.t1) return t.sb[p - t.base];
    return t.g[p];
}

__device__ __forceinline__ u64 ix_klen(const Rec& x) { return (x.ref >> 40) & LONG_LEN_MAX; }

// the count of the line [s, s + len) whose key k_line_recs measured as klen bytes: -1 and *v set,
// or the rule it breaks (IX_COUNT, IX_ZERO)
template <bool STAGED>
__device__ __forceinline__ int ix_parse(const IxText& t, u64 s, u64 len, u64 klen, u64* v) {
    *v = 0;
    const u64 e = s + len;
    if (len < 5 || ix_byte<STAGED>(t, e - 1) != '\n') return IX_COUNT;   // "k: 1\n" is the shortest line
    u32 nd = 0;
    u64 p = e - 1;                                   // digits, backwards, never before the line's start
    while (nd < 21 && p > s) {
        const u32 b = ix_byte<STAGED>(t, p - 1);
        if (b < '0' || b > '9') break;
        nd++;
        p--;
    }
    if (nd == 0 || nd > 20) return IX_COUNT;
    if (klen == 0 || len != klen + 3 + nd) return IX_COUNT;              // now p == s + klen + 2
    if (ix_byte<STAGED>(t, p - 2) != ':' || ix_byte<STAGED>(t, p - 1) != ' ') return IX_COUNT;
    if (ix_byte<STAGED>(t, p) == '0') return nd == 1 ? IX_ZERO : IX_COUNT;
    u64 c = 0;
    for (u32 j = 0; j < nd && j < 19; j++) c = c * 10 + (ix_byte<STAGED>(t, p + j) - '0');
    if (nd == 20) {
        const u32 d = ix_byte<STAGED>(t, p + 19) - '0';
        if (c > IX_U64_DIV10 || (c == IX_U64_DIV10 && d > 5)) return IX_COUNT;
        c = c * 10 + d;
    }
    *v = c;
    return -1;
}

// does record x (text at xs) sort strictly after record p (text at ps)?  The prefixes decide first;
// equal prefixes of two long keys: the bytes from 16 on, then the lengths; equal prefixes otherwise:
// the shorter key's padding met zeros, so it is a prefix of the other and the lengths decide.
template <bool STAGED>
__device__ __forceinline__ bool ix_after(const IxText& t, const Rec& p, u64 ps, const Rec& x, u64 xs) {
    if (p.hi != x.hi) return p.hi < x.hi;
    if (p.lo != x.lo) return p.lo < x.lo;
    const u64 pl = ix_klen(p), xl = ix_klen(x);
    if (pl >= 16 && xl >= 16) {
        const u64 m = pl < xl ? pl : xl;
        for (u64 k = 16; k < m; k++) {
            const u32 a = ix_byte<STAGED>(t, ps + k), b = ix_byte<STAGED>(t, xs + k);
            if (a != b) return a < b;
        }
    }
    return pl < xl;
}

// a thread's FM_IPT lines x[] (records i0 ..., the first at text offset st), after record prev
template <bool STAGED>
__device__ __forceinline__ void ix_lines(const IxText& t, const Rec* x, Rec prev, u64 i0, u64 n, u64 st, Rec* out,
                                         u64* err) {
    u64 ps = i0 ? st - prev.cnt : 0;
    for (int k = 0; k < FM_IPT; k++) {
        const u64 i = i0 + k;
        if (i >= n) break;
        const u64 klen = ix_klen(x[k]);
        Rec q;
        q.hi = x[k].hi; q.lo = x[k].lo;
        q.ref = klen < 16 ? klen : LONG_FLAG | (klen << 40) | st;
        const int bad = ix_parse<STAGED>(t, st, x[k].cnt, klen, &q.cnt);
        if (bad >= 0) atomicMin((unsigned long long*)&err[bad], (unsigned long long)i);
        if (i && !ix_after<STAGED>(t, prev, ps, x[k], st)) atomicMin((unsigned long long*)&err[IX_ORDER], (unsigned long long)i);
        out[i] = q;
        prev = x[k];
        ps = st;
        st += x[k].cnt;
    }
}

// the line of the tile that holds text byte p: starts[0, m) ascending, starts[0] <= p
__device__ __forceinline__ u32 ix_line_of(const u64* starts, u32 m, u64 p) {
    u32 lo = 0, hi = m;                              // the last j with starts[j] <= p
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (starts[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool ix_has_zero(u32 w) { return ((w - 0x01010101u) & ~w & 0x80808080u) != 0; }

// r[0, n): the line records, n >= 1; text[0, text_len): their lines back to back; toff: the tiles'
// offsets (k_ix_sum, scanned); out[0, n): the query records; err[IX_KINDS]: preset to IX_NONE.
// stage <= FM_STAGE: tiles of at most this many bytes (alignment padding included) go through LDS.
__global__ __launch_bounds__(FM_NT) void k_ix_write(const Rec* __restrict__ r, u64 n, const uint8_t* __restrict__ text,
                                                   u64 text_len, const u64* __restrict__ toff, Rec* __restrict__ out,
                                                   u64* err, u32 stage) {
    __shared__ u64 ws[FM_NT / 64];
    __shared__ u64 starts[FM_TILE];
    __shared__ u32 nul_line;
    __shared__ __align__(16) uint8_t sb[FM_STAGE];
    const u32 tid = threadIdx.x;
    const u64 tile0 = (u64)blockIdx.x * FM_TILE, i0 = tile0 + (u64)tid * FM_IPT;
    Rec x[FM_IPT];
    fmt_load(r, n, i0, x);
    const Rec prev = r[i0 ? (i0 - 1 < n ? i0 - 1 : n - 1) : 0];
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < FM_IPT; k++) {
        if (i0 + k >= n) x[k].cnt = 0;
        s += x[k].cnt;
    }
    u64 all;
    const u64 lo = block_excl_scan(s, ws, all);
    const u64 t0 = toff[blockIdx.x];
    {
        u64 st = t0 + lo;
#pragma unroll
        for (int k = 0; k < FM_IPT; k++) { starts[tid * FM_IPT + k] = st; st += x[k].cnt; }
    }
    if (tid == 0) nul_line = ~0u;
    __syncthreads();
    if (t0 + all > text_len || t0 + all < t0) {      // workgroup-uniform; not records of this text
        if (tid == 0) atomicMin((unsigned long long*)&err[IX_COUNT], (unsigned long long)tile0);
        return;
    }
    // the tile's text, once: zero bytes found (and, staged, the bytes kept) on the way.  Chunk c is
    // the 16 aligned bytes at text + t0 - pad + 16 c; the edges go bytewise.
    const u32 pad = (u32)((uintptr_t)(text + t0) & 15);
    const bool staged = pad + all <= stage;          // workgroup-uniform
    const u64 total = pad + all;
    const uint8_t* const base = text + t0 - pad;     // (never dereferenced below base + pad)
    const u32 m = (u32)(n - tile0 < FM_TILE ? n - tile0 : FM_TILE);
    for (u64 b0 = 16ull * tid; b0 < total; b0 += 16ull * FM_NT) {
        const u64 b1 = b0 + 16 < total ? b0 + 16 : total;
        bool z = false;
        if (b0 >= pad && b1 == b0 + 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(base + b0);
            if (staged) *reinterpret_cast<uint4*>(sb + b0) = v;
            z = ix_has_zero(v.x) | ix_has_zero(v.y) | ix_has_zero(v.z) | ix_has_zero(v.w);
        } else {
            for (u64 b = b0 > pad ? b0 : pad; b < b1; b++) {
                const uint8_t v = base[b];
                if (staged) sb[b] = v;
                z |= v == 0;
            }
        }
        if (z) {                                     // the error path: which line?
            for (u64 b = b0 > pad ? b0 : pad; b < b1; b++)
                if (base[b] == 0) { atomicMin(&nul_line, ix_line_of(starts, m, t0 - pad + b)); break; }
        }
    }
    __syncthreads();
    if (tid == 0 && nul_line != ~0u) atomicMin((unsigned long long*)&err[IX_NUL], (unsigned long long)(tile0 + nul_line));
    IxText t;
    t.g = text; t.sb = sb; t.base = t0 - pad; t.t0 = t0; t.t1 = t0 + all;
    if (staged) ix_lines<true>(t, x, prev, i0, n, t0 + lo, out, err);
    else ix_lines<false>(t, x, prev, i0, n, t0 + lo, out, err);
}

}  // namespace wcg
