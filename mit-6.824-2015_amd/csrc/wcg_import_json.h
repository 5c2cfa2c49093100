// wcg_import_json.h - the reference's JSON files read on the device (wcg_import_json), on gfx950.
//
// Both files are lines {"Key":"<key>","Value":"<value>"}\n.  DoMap's intermediates mrtmp.<f>-<m>-<r>
// (mapreduce.go:214-230) carry one line per occurrence with the value "1" (IJ_MAP); DoReduce's
// mrtmp.<f>-res-<r> (mapreduce.go:264-279) one line per key with its count (IJ_RES).
//
// The text is cut into tiles of IJ_TILE bytes, one workgroup each, IJ_SPAN consecutive bytes per
// thread.  A line belongs to the tile (and the thread) that holds its '\n'.
//
//   k_ij_nl     per tile: its '\n' count and the position after its last '\n' (0: none).
//               k_scan_u64 turns the counts into each tile's first line number, k_ij_maxscan the
//               positions into each tile's first line START (the running maximum of the earlier
//               tiles): no thread ever searches backwards for a newline.
//   k_ij_check  the tile staged in LDS by 16-byte loads; every line that ends in it is checked
//               against the rules below; per tile the output size (MAP: bytes of "key\n" text,
//               RES: 32-byte exchange units).  k_scan_u64 makes the output offsets.
//   k_ij_keys   MAP: the keys compacted to "key\n" text (what the context then maps through the
//               path of wcg_map_device: hot keys pre-aggregate in LDS).
//   k_ij_units  RES: exchange units as k_export_write writes them (an inline Rec for keys of <= 15
//               bytes; a LONG_FLAG header + ceil(len / 24) CONT_MARK units otherwise), for k_import.
//
// Rules per line (B = the line without its '\n', L = its length), the first broken one reported:
//   frame  L >= 10, B starts with {"Key":" and ends with "}
//   value  V = the run of bytes other than '"' that ends at L-2, followed back for at most 21 bytes
//          and never into B[0..8): not empty, closed by a '"' within those bounds; MAP: V is "1";
//          RES: V is a canonical decimal in 1 .. 2^64-1 (first digit 1-9, at most 20 digits)
//   sep    the 11 bytes that end with V's opening quote are ","Value":" and begin at offset >= 8
//   key    K = B[8 .. L-2-len(V)-11) has 1 .. 2^23-1 bytes, every rune valid UTF-8 (go_decode) and a
//          letter (lt_is_letter): Go's tokenizer returns exactly K for K
// A broken rule is reported, never a fault: err[rule] = the lowest offending line (atomicMin, which
// only the error path touches).  A line reports its first broken rule only, so the host takes the
// lowest line of the four words.
//
// Bounds.  The host refuses a text whose last byte is not '\n', so every byte lies in a line that
// ends at a '\n' inside [0, n).  A line's start s is 0 or a '\n' position + 1 (from the scans
// above), its end e a '\n' position: 0 <= s <= e < n, and every read of a line is of a byte in
// [s, e): ij_line reads B[j] only after comparing j with L (frame: L >= 10 before B[0..8) and
// B[L-2..L); value: positions L-3 down to 8; sep: positions q-10 .. q with q-10 >= 8; key:
// [8, q-10), the decoder's look-ahead answered with 0 past the key's end).  Tile reads: 16-byte
// chunks only where the whole chunk lies below n, single bytes below n otherwise; positions at or
// past n stage as 0.  Writes: a tile writes exactly the size it reported to the scan, starting at
// its scanned offset (k_ij_keys: sum of L+1-22 over its lines; k_ij_units: sum of units), so
// nothing is written at or past the scanned total, which the host allocated.
#pragma once
#include "wcg_common.h"
#include "wcg_index.h"
#include "wcg_reduce.h"

namespace wcg {

constexpr int IJ_MAP = 0, IJ_RES = 1;
constexpr int IJ_FRAME = 0, IJ_VALUE = 1, IJ_SEP = 2, IJ_KEY = 3, IJ_KINDS = 4;
constexpr int IJ_NT = 256;
constexpr u32 IJ_SPAN = 64;                        // bytes per thread: one 64-bit newline mask
constexpr u32 IJ_TILE = 16384;                     // = IJ_NT * IJ_SPAN
constexpr u64 IJ_MAP_FIXED = 22;                   // line bytes with '\n' - ("key\n" bytes): 8 + 11 + 1 + 2 + 1 - 1
static_assert(IJ_TILE == IJ_NT * IJ_SPAN, "a thread owns IJ_SPAN consecutive bytes of its tile");

// zero bytes of w as bits 7, 15, 23, 31 (exact: no borrow crosses a byte)
__device__ __forceinline__ u32 ij_zero_mask(u32 w) {
    const u32 t = (w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | w | 0x7F7F7F7Fu);
}
// '\n' bytes of the little-endian dword w as bits 0 .. 3
__device__ __forceinline__ u32 ij_nl4(u32 w) {
    const u32 z = ij_zero_mask(w ^ 0x0A0A0A0Au);
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
__device__ __forceinline__ u32 ij_nl16(const uint4& v) {
    return ij_nl4(v.x) | ij_nl4(v.y) << 4 | ij_nl4(v.z) << 8 | ij_nl4(v.w) << 12;
}

// the 16 bytes of the text at p (a multiple of 16 from the text's start); bytes at or past n are 0
__device__ __forceinline__ uint4 ij_chunk(const uint8_t* __restrict__ text, u64 n, u64 p, bool aligned) {
    if (aligned && p + 16 <= n) return *reinterpret_cast<const uint4*>(text + p);
    u32 w[4] = {0, 0, 0, 0};
    for (u32 k = 0; k < 16; k++)
        if (p + k < n) w[k >> 2] |= (u32)text[p + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// cnt[b] = the '\n' bytes of tile b, last[b] = the position after its last one (0: none)
__global__ __launch_bounds__(IJ_NT) void k_ij_nl(const uint8_t* __restrict__ text, u64 n, u64* __restrict__ cnt,
                                                u64* __restrict__ last) {
    __shared__ u64 wc[IJ_NT / 64], wl[IJ_NT / 64];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * IJ_TILE;
    const bool aligned = ((uintptr_t)text & 15) == 0;
    u64 c = 0, l = 0;
#pragma unroll
    for (u32 k = 0; k < IJ_TILE / 16 / IJ_NT; k++) {
        const u64 p = t0 + 16ull * (k * IJ_NT + tid);
        if (p >= n) continue;
        const u32 m = ij_nl16(ij_chunk(text, n, p, aligned));
        c += __popc(m);
        if (m) l = p + (32 - __clz(m));              // ascending p: the last one stays
    }
    for (int d = 32; d; d >>= 1) {
        c += __shfl_xor(c, d, 64);
        const u64 y = __shfl_xor(l, d, 64);
        l = y > l ? y : l;
    }
    if ((tid & 63) == 0) { wc[tid >> 6] = c; wl[tid >> 6] = l; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < IJ_NT / 64; k++) { c += wc[k]; l = wl[k] > l ? wl[k] : l; }
        cnt[blockIdx.x] = c;
        last[blockIdx.x] = l;
    }
}

// v[i] = max(v[0 .. i)) in place (0 for i = 0): one workgroup
__global__ __launch_bounds__(1024) void k_ij_maxscan(u64* v, u64 n) {
    __shared__ u64 ws[16];
    __shared__ u64 carry_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (u64 base = 0; base < n; base += 1024) {
        const u64 i = base + tid;
        const u64 x = i < n ? v[i] : 0;
        u64 incl = x;
        for (int d = 1; d < 64; d <<= 1) { const u64 y = __shfl_up(incl, d, 64); if (lane >= d && y > incl) incl = y; }
        u64 excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0;
        if (lane == 63) ws[w] = incl;
        __syncthreads();
        u64 pre = carry_s, all = carry_s;
        for (int k = 0; k < 16; k++) { if (k < w && ws[k] > pre) pre = ws[k]; if (ws[k] > all) all = ws[k]; }
        if (i < n) v[i] = excl > pre ? excl : pre;
        __syncthreads();
        if (tid == 0) carry_s = all;
        __syncthreads();
    }
}

// the text as a line's code reads it: g[p] for any p < t1; the staged tile has sb[p - t0] == g[p]
// for t0 <= p (every position a tile's lines read lies below the tile's end)
struct IjText {
    const uint8_t* g;
    const uint8_t* sb;
    u64 t0;
};
__device__ __forceinline__ u32 ij_byte(const IjText& t, u64 p) { return p >= t.t0 ? t.sb[p - t.t0] : t.g[p]; }

// a checked line: the key is B[8, 8 + klen), the count cnt
struct IjLine {
    u64 klen, cnt;
};

// the line [s, e) (e: its '\n'): -1 and *o set, or the first rule it breaks
__device__ __forceinline__ int ij_line(const IjText& t, u64 s, u64 e, int mode, IjLine* o) {
    const u64 L = e - s;
    if (L < 10) return IJ_FRAME;
    {
        const char* pre = "{\"Key\":\"";
        bool ok = true;
        for (int k = 0; k < 8; k++) ok &= ij_byte(t, s + k) == (u32)pre[k];
        ok &= ij_byte(t, e - 2) == '"' && ij_byte(t, e - 1) == '}';
        if (!ok) return IJ_FRAME;
    }
    // V: back from B[L-3], at most 21 bytes, never into B[0..8); q = its opening quote
    u32 vl = 0;
    while (vl < 21 && L - 3 - vl >= 8 && ij_byte(t, e - 3 - vl) != '"') vl++;
    if (L - 3 - vl < 8 || ij_byte(t, e - 3 - vl) != '"') return IJ_VALUE;
    if (vl == 0) return IJ_VALUE;
    const u64 q = L - 3 - vl;                        // offset in B, >= 8
    u64 c = 0;
    if (mode == IJ_MAP) {
        if (vl != 1 || ij_byte(t, e - 3) != '1') return IJ_VALUE;
        c = 1;
    } else {
        if (vl > 20) return IJ_VALUE;
        const u64 v0 = s + q + 1;
        for (u32 j = 0; j < vl; j++) {
            const u32 d = ij_byte(t, v0 + j) - '0';
            if (d > 9 || (j == 0 && d == 0)) return IJ_VALUE;
            if (j == 19 && (c > IX_U64_DIV10 || (c == IX_U64_DIV10 && d > 5))) return IJ_VALUE;
            c = c * 10 + d;
        }
    }
    if (q < 18) return IJ_SEP;                       // the 11 bytes would begin before offset 8
    {
        const char* sep = "\",\"Value\":\"";
        bool ok = true;
        for (int k = 0; k < 11; k++) ok &= ij_byte(t, s + q - 10 + k) == (u32)sep[k];
        if (!ok) return IJ_SEP;
    }
    const u64 klen = q - 18;
    if (klen == 0 || klen > LONG_LEN_MAX) return IJ_KEY;
    const u64 k0 = s + 8, k1 = k0 + klen;
    auto at = [&](long p) -> u32 { return (u64)p < k1 ? ij_byte(t, (u64)p) : 0u; };
    for (u64 p = k0; p < k1;) {
        const u32 b = ij_byte(t, p);
        if (b < 0x80) {
            if (((b | 0x20) - 'a') >= 26u) return IJ_KEY;
            p++;
            continue;
        }
        u32 cp;
        const int w = go_decode(at, (long)p, &cp);
        if (w == 0 || !lt_is_letter(cp)) return IJ_KEY;
        p += w;
    }
    o->klen = klen;
    o->cnt = c;
    return -1;
}

__device__ __forceinline__ u64 ij_units(u64 klen) { return klen <= 15 ? 1 : 1 + (klen + CONT_BYTES - 1) / CONT_BYTES; }

// what every pass over the lines shares: the tile staged in sb, this thread's '\n' mask (bit j:
// position t0 + IJ_SPAN * tid + j), the number of the tile's lines before its first one and the
// start of its first line.  ws: 2 * IJ_NT / 64 words.
struct IjThread {
    u64 mask, line0, start;
};
__device__ __forceinline__ IjThread ij_stage(const uint8_t* __restrict__ text, u64 n, u64 t0, const u64* __restrict__ line_off,
                                             const u64* __restrict__ start_of, uint8_t* sb, u64* ws) {
    const u32 tid = threadIdx.x;
    const bool aligned = ((uintptr_t)text & 15) == 0;
#pragma unroll
    for (u32 k = 0; k < IJ_TILE / 16 / IJ_NT; k++) {
        const u32 c = k * IJ_NT + tid;
        const u64 p = t0 + 16ull * c;
        *reinterpret_cast<uint4*>(sb + 16 * c) = p < n ? ij_chunk(text, n, p, aligned) : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    u64 m = 0;
#pragma unroll
    for (u32 k = 0; k < IJ_SPAN / 16; k++)
        m |= (u64)ij_nl16(*reinterpret_cast<const uint4*>(sb + IJ_SPAN * tid + 16 * k)) << (16 * k);
    const u64 cnt = __popcll(m);
    const u64 last = m ? t0 + (u64)IJ_SPAN * tid + (64 - __clzll(m)) : 0;   // the position after this thread's last '\n'
    const int lane = tid & 63, w = tid >> 6;
    u64 ic = cnt, il = last;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 yc = __shfl_up(ic, d, 64), yl = __shfl_up(il, d, 64);
        if (lane >= d) { ic += yc; il = yl > il ? yl : il; }
    }
    u64 el = __shfl_up(il, 1, 64);
    if (lane == 0) el = 0;
    if (lane == 63) { ws[w] = ic; ws[IJ_NT / 64 + w] = il; }
    __syncthreads();
    u64 pc = 0, pl = start_of[blockIdx.x];
    for (int k = 0; k < IJ_NT / 64; k++)
        if (k < w) { pc += ws[k]; pl = ws[IJ_NT / 64 + k] > pl ? ws[IJ_NT / 64 + k] : pl; }
    IjThread r;
    r.mask = m;
    r.line0 = line_off[blockIdx.x] + pc + ic - cnt;
    r.start = el > pl ? el : pl;
    return r;
}

// sum over the workgroup (every thread gets it); ws: IJ_NT / 64 words, free to reuse after the call
__device__ __forceinline__ u64 ij_block_sum(u64 v, u64* ws) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 all = 0;
    for (int k = 0; k < IJ_NT / 64; k++) all += ws[k];
    __syncthreads();
    return all;
}

// out_size[b] = the output of tile b's lines (MAP: bytes, RES: units); err[IJ_KINDS] preset to ~0
__global__ __launch_bounds__(IJ_NT) void k_ij_check(const uint8_t* __restrict__ text, u64 n, int mode,
                                                   const u64* __restrict__ line_off, const u64* __restrict__ start_of,
                                                   u64* __restrict__ out_size, u64* err) {
    __shared__ u64 ws[2 * IJ_NT / 64];
    __shared__ __align__(16) uint8_t sb[IJ_TILE];
    const u64 t0 = (u64)blockIdx.x * IJ_TILE;
    const IjThread th = ij_stage(text, n, t0, line_off, start_of, sb, ws);
    IjText t;
    t.g = text; t.sb = sb; t.t0 = t0;
    u64 m = th.mask, s = th.start, line = th.line0, size = 0;
    while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const u64 e = t0 + (u64)IJ_SPAN * threadIdx.x + j;
        IjLine o;
        const int bad = ij_line(t, s, e, mode, &o);
        if (bad >= 0) atomicMin((unsigned long long*)&err[bad], (unsigned long long)line);
        else size += mode == IJ_MAP ? o.klen + 1 : ij_units(o.klen);
        s = e + 1;
        line++;
    }
    const u64 all = ij_block_sum(size, ws);
    if (threadIdx.x == 0) out_size[blockIdx.x] = all;
}

// MAP, after a clean k_ij_check: "key\n" for every line, in file order, at out + out_off[tile].
// A tile whose keys fit the stage goes through LDS and leaves in aligned 16-byte stores.
__global__ __launch_bounds__(IJ_NT) void k_ij_keys(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line_off,
                                                  const u64* __restrict__ start_of, const u64* __restrict__ out_off,
                                                  uint8_t* __restrict__ out) {
    __shared__ u64 ws[2 * IJ_NT / 64];
    __shared__ __align__(16) uint8_t sb[IJ_TILE];
    __shared__ __align__(16) uint8_t ob[IJ_TILE + 16];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * IJ_TILE;
    const IjThread th = ij_stage(text, n, t0, line_off, start_of, sb, ws);
    IjText t;
    t.g = text; t.sb = sb; t.t0 = t0;
    // this thread's lines are [th.start, the position after its last '\n'): every one sheds 22 bytes
    const u64 nl = __popcll(th.mask);
    const u64 mine = nl ? t0 + (u64)IJ_SPAN * tid + (64 - __clzll(th.mask)) - th.start - IJ_MAP_FIXED * nl : 0;
    __syncthreads();                                 // ij_stage's readers of ws are done
    u64 all;
    const u64 lo = block_excl_scan(mine, ws, all);
    uint8_t* const dst = out + out_off[blockIdx.x];
    const u32 pad = (u32)((uintptr_t)dst & 15);
    const bool staged = all <= IJ_TILE;              // workgroup-uniform
    uint8_t* o = staged ? ob + pad + lo : dst + lo;
    u64 m = th.mask, s = th.start;
    while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const u64 e = t0 + (u64)IJ_SPAN * tid + j;
        const u64 klen = e - s - (IJ_MAP_FIXED + 1) + 1;   // L - 22
        for (u64 k = 0; k < klen; k++) *o++ = (uint8_t)ij_byte(t, s + 8 + k);
        *o++ = '\n';
        s = e + 1;
    }
    if (!staged) return;
    __syncthreads();
    uint8_t* const base = dst - pad;                 // 16-byte aligned; ob[b] is base[b]
    const u32 total = pad + (u32)all;
    for (u32 c = tid; 16 * c < total; c += IJ_NT) {
        const u32 b0 = 16 * c, b1 = b0 + 16 < total ? b0 + 16 : total;
        if (b0 >= pad && b1 == b0 + 16) *reinterpret_cast<uint4*>(base + b0) = *reinterpret_cast<const uint4*>(ob + b0);
        else for (u32 b = b0 > pad ? b0 : pad; b < b1; b++) base[b] = ob[b];
    }
}

// the value's opening quote of a checked RES line, as an offset in B (ij_line's q), and its count
__device__ __forceinline__ u64 ij_res_value(const IjText& t, u64 s, u64 e, u64* cnt) {
    u32 vl = 0;
    while (vl < 20 && ij_byte(t, e - 3 - vl) != '"') vl++;     // checked: 1 .. 20 digits, then the quote
    u64 c = 0;
    for (u32 j = 0; j < vl; j++) c = c * 10 + (ij_byte(t, e - 2 - vl + j) - '0');
    *cnt = c;
    return e - s - 3 - vl;
}

// RES, after a clean k_ij_check: the exchange units of every line at out + out_off[tile]
__global__ __launch_bounds__(IJ_NT) void k_ij_units(const uint8_t* __restrict__ text, u64 n, const u64* __restrict__ line_off,
                                                   const u64* __restrict__ start_of, const u64* __restrict__ out_off,
                                                   Rec* __restrict__ out) {
    __shared__ u64 ws[2 * IJ_NT / 64];
    __shared__ __align__(16) uint8_t sb[IJ_TILE];
    const u32 tid = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * IJ_TILE;
    const IjThread th = ij_stage(text, n, t0, line_off, start_of, sb, ws);
    IjText t;
    t.g = text; t.sb = sb; t.t0 = t0;
    u64 mine = 0;
    {
        u64 m = th.mask, s = th.start;
        while (m) {
            const int j = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const u64 e = t0 + (u64)IJ_SPAN * tid + j;
            u64 c;
            mine += ij_units(ij_res_value(t, s, e, &c) - 18);
            s = e + 1;
        }
    }
    __syncthreads();                                 // ij_stage's readers of ws are done
    u64 all;
    u64 pos = out_off[blockIdx.x] + block_excl_scan(mine, ws, all);
    u64 m = th.mask, s = th.start;
    while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const u64 e = t0 + (u64)IJ_SPAN * tid + j;
        Rec h;
        const u64 klen = ij_res_value(t, s, e, &h.cnt) - 18;
        const u64 k0 = s + 8;
        h.hi = h.lo = 0;
        for (u64 k = 0; k < klen && k < 16; k++) {
            const u64 b = ij_byte(t, k0 + k);
            if (k < 8) h.hi |= b << (56 - 8 * k);
            else h.lo |= b << (120 - 8 * k);
        }
        if (klen <= 15) {
            h.ref = klen;
            out[pos++] = h;
        } else {
            h.ref = LONG_FLAG | (klen << 40);
            out[pos++] = h;
            for (u64 c0 = 0; c0 < klen; c0 += CONT_BYTES) {
                u64 w[3] = {0, 0, 0};
                for (int k = 0; k < CONT_BYTES; k++) {
                    const u64 b = c0 + k < klen ? ij_byte(t, k0 + c0 + k) : 0;
                    w[k >> 3] |= b << (8 * (k & 7));
                }
                Rec cr;
                cr.hi = w[0]; cr.lo = w[1]; cr.cnt = w[2]; cr.ref = CONT_MARK;
                out[pos++] = cr;
            }
        }
        s = e + 1;
    }
}

}  // namespace wcg
