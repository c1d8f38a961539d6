// Packed emission windows (format version 1, INTEGRATION.md "Packed windows"): more than 97 % of a witness' canonical 32-byte values are the numbers 0 and 1, so a window
// crosses PCIe as 2-bit tags + the few values that are neither (reference: writeBinWitness, patch point tests/test.py:36, writes 32 bytes per wire).
//   device:  launch_pack_window -- four launches behind everything that writes the canonical window (pob_host.hip emit_make_window), in front of its copy
//   host:    pob_unpack_window  -- validates a packed window and expands it to canonical values on the loader's thread pool (pack_json.hip); no GPU touched
//
//   header 32 B   u32 magic 'POBP', u32 version 1, u64 first_wire, u32 n_wires, u32 n_small, u32 n_wide, u32 0
//   tag planes    ceil(n / 64) x {u64 lo, u64 hi}: bit i % 64 of pair i / 64 = wire i's tag hi << 1 | lo -- 0: value 0, 1: value 1, 2: 2 <= value < 2^32, 3: anything else
//   chunk index   ceil(n / 4096) x {u32 small_before, u32 wide_before}
//   small values  n_small x u32, wire order
//   wide values   n_wide x 32 B, wire order
// every section starts on a 32-byte boundary, padding is zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <functional>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/pob_hip.h"
#include "pack_window.hpp"

typedef unsigned long long u64;
#define PK_MAGIC 0x50424F50u          // "POBP", little-endian
#define PK_VERSION 1u

static __host__ __device__ inline uint64_t pk_pad32(uint64_t b) { return (b + 31) & ~(uint64_t)31; }
static __host__ __device__ inline uint64_t pk_idx_off(uint64_t n) { return 32 + pk_pad32(16 * ((n + 63) / 64)); }
static __host__ __device__ inline uint64_t pk_fixed(uint64_t n) { return pk_idx_off(n) + pk_pad32(8 * ((n + 4095) / 4096)); }
uint64_t pack_fixed_bytes(uint64_t n) { return pk_fixed(n); }
uint64_t pack_value_bytes(uint64_t n_small, uint64_t n_wide) { return pk_pad32(4 * n_small) + 32 * n_wide; }

// ---- classification: lane = wire, one wavefront per 64 positions (2 KB contiguous as two 16-byte loads per lane); two ballots are the block's lo / hi words
__global__ void __launch_bounds__(256) k_pack_classify(const uint4* win, uint32_t n, uint4* planes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t tag = 0;                                   // positions beyond n: tag 0, their plane bits stay zero
    if (i < n) {
        const uint4 a = win[2 * i], b = win[2 * i + 1];
        const bool narrow = (a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
        tag = !narrow ? 3u : a.x < 2u ? a.x : 2u;
    }
    const u64 lo = __ballot((tag & 1u) != 0), hi = __ballot((tag >> 1) != 0);
    if ((threadIdx.x & 63u) == 0 && i < n) planes[i >> 6] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// ---- offsets, first level: one wavefront per chunk of 64 blocks (4 096 positions); lane = block.  blk_pre[b] = small | wide << 16 in front of block b inside its
// chunk (both <= 4 096), chunk_tot[c] = the chunk's counts in the same form
__global__ void __launch_bounds__(64) k_pack_scan_chunk(const u64* planes, uint32_t nblk, uint32_t* blk_pre, uint32_t* chunk_tot) {
    const uint32_t lane = threadIdx.x & 63u, b = blockIdx.x * 64 + lane;
    uint32_t c = 0;
    if (b < nblk) { const u64 lo = planes[2 * (uint64_t)b], hi = planes[2 * (uint64_t)b + 1]; c = (uint32_t)__popcll(hi & ~lo) | (uint32_t)__popcll(hi & lo) << 16; }
    uint32_t inc = c;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl(inc, (lane - d) & 63u, 64); if (lane >= d) inc += t; }
    if (b < nblk) blk_pre[b] = inc - c;
    if (lane == 63) chunk_tot[blockIdx.x] = inc;
}

// ---- offsets, second level: ONE wavefront scans the chunks' counts (2 048 at the default window: 32 steps) and writes the chunk index, the header and the padding
__global__ void __launch_bounds__(64) k_pack_scan_top(uint8_t* pk, uint64_t first_wire, uint32_t n, const uint32_t* chunk_tot) {
    const uint32_t lane = threadIdx.x & 63u, nblk = (n + 63) / 64, nchunk = (n + 4095) / 4096;
    uint32_t* idx = (uint32_t*)(pk + pk_idx_off(n));
    uint32_t cs = 0, cw = 0;
    for (uint32_t base = 0; base < nchunk; base += 64) {
        const uint32_t c = base + lane, t = c < nchunk ? chunk_tot[c] : 0, s = t & 0xFFFFu, w = t >> 16;
        uint32_t is = s, iw = w;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t ts = __shfl(is, (lane - d) & 63u, 64), tw = __shfl(iw, (lane - d) & 63u, 64);
            if (lane >= d) { is += ts; iw += tw; }
        }
        if (c < nchunk) { idx[2 * (uint64_t)c] = cs + is - s; idx[2 * (uint64_t)c + 1] = cw + iw - w; }
        cs += __shfl(is, 63, 64); cw += __shfl(iw, 63, 64);
    }
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        ((uint4*)pk)[0] = make_uint4(PK_MAGIC, PK_VERSION, (uint32_t)first_wire, (uint32_t)(first_wire >> 32));
        ((uint4*)pk)[1] = make_uint4(n, cs, cw, 0);
    }
    if (lane == 1 && (nblk & 1u)) ((uint4*)(pk + 32))[nblk] = zero;                                   // behind an odd number of 16-byte plane pairs
    const uint32_t ipad = (uint32_t)((pk_pad32(8 * (uint64_t)nchunk) - 8 * (uint64_t)nchunk) / 4);   // <= 6 words behind the chunk index
    if (lane < ipad) idx[2 * (uint64_t)nchunk + lane] = 0;
    const uint32_t spad = (uint32_t)((pk_pad32(4 * (uint64_t)cs) - 4 * (uint64_t)cs) / 4);           // <= 7 words behind the small values
    if (lane < spad) ((uint32_t*)(pk + pk_fixed(n)))[(uint64_t)cs + lane] = 0;
}

// ---- scatter: a wire that is neither 0 nor 1 lands at chunk index + block prefix + its rank among the lower lanes of its block; tags come from the planes (no second
// classification), so only those wires -- under 3 % -- are read again
__global__ void __launch_bounds__(256) k_pack_scatter(const uint4* win, uint32_t n, uint8_t* pk, const uint32_t* blk_pre) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = i >> 6; const uint32_t lane = (uint32_t)i & 63u;
    const u64* planes = (const u64*)(pk + 32);
    const u64 lo = planes[2 * b], hi = planes[2 * b + 1];
    if (!((hi >> lane) & 1)) return;
    const uint32_t* idx = (const uint32_t*)(pk + pk_idx_off(n));
    const uint32_t pre = blk_pre[b];
    const u64 below = ((u64)1 << lane) - 1;
    uint8_t* vals = pk + pk_fixed(n);
    if (!((lo >> lane) & 1)) {
        const uint64_t r = (uint64_t)idx[2 * (i >> 12)] + (pre & 0xFFFFu) + (uint32_t)__popcll(hi & ~lo & below);
        ((uint32_t*)vals)[r] = win[2 * i].x;
    } else {
        const uint32_t n_small = ((const uint32_t*)pk)[5];
        const uint64_t r = (uint64_t)idx[2 * (i >> 12) + 1] + (pre >> 16) + (uint32_t)__popcll(hi & lo & below);
        uint4* dst = (uint4*)(vals + pk_pad32(4 * (uint64_t)n_small)) + 2 * r;
        dst[0] = win[2 * i]; dst[1] = win[2 * i + 1];
    }
}

void launch_pack_window(const uint8_t* win, uint64_t first_wire, uint32_t n, uint8_t* pk, uint32_t* blk_pre, uint32_t* chunk_tot, hipStream_t st) {
    const uint32_t nblk = (n + 63) / 64, nchunk = (n + 4095) / 4096, grid = (n + 255) / 256;
    const uint4* w4 = (const uint4*)win; uint4* planes4 = (uint4*)(pk + 32); const u64* planes = (const u64*)(pk + 32);      // (plain locals: the CPU shim's launch macro evaluates its arguments inside a by-copy lambda)
    const uint32_t* tot = chunk_tot; const uint32_t* pre = blk_pre;
    hipLaunchKernelGGL(k_pack_classify, dim3(grid), dim3(256), 0, st, w4, n, planes4);
    hipLaunchKernelGGL(k_pack_scan_chunk, dim3(nchunk), dim3(64), 0, st, planes, nblk, blk_pre, chunk_tot);
    hipLaunchKernelGGL(k_pack_scan_top, dim3(1), dim3(64), 0, st, pk, first_wire, n, tot);
    hipLaunchKernelGGL(k_pack_scatter, dim3(grid), dim3(256), 0, st, w4, n, pk, pre);
}

// ------------------------------------------------------------------------------------------------ the pack pass over the 64 windows of a group emission
// The four kernels above with a witness dimension: blockIdx.y = rank of the witness among the selected ones (an unselected witness launches nothing); canonical window at
// win + l * plane, packed form at pk + l * pk_stride, scratch rows blk_pre[l][nblk] and chunk_tot[l][nchunk].  The blocks that the Keccak runs' direct route wrote
// (k_emit_group.hip: plane words in place, hi = 0, no canonical form) are not launched over at all: fill, classification and scatter run over the block ranges
// [b0, b1) BETWEEN them, which the host knows; the scan reads the planes only and counts nothing for a direct block.
__device__ __forceinline__ uint32_t pk_lane_of_rank(u64 lanes, uint32_t r) { for (uint32_t k = 0; k < r; k++) lanes &= lanes - 1; return (uint32_t)__builtin_ctzll(lanes); }
__global__ void __launch_bounds__(256) k_fill_ee_group(PackGroup g, uint32_t p0, uint32_t p1, bool one_at_0) {
    const uint32_t l = pk_lane_of_rank(g.lanes, blockIdx.y);
    const uint64_t i = (uint64_t)p0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p1) return;
    uint4* q = (uint4*)(g.win + (uint64_t)l * g.plane) + 2 * i;
    if (i == 0 && one_at_0) { q[0] = make_uint4(1, 0, 0, 0); q[1] = make_uint4(0, 0, 0, 0); return; }       // wire 0 of the payload is the constant 1
    q[0] = q[1] = make_uint4(0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu);
}
// p0 is a multiple of 64: a wavefront is one block of the window; p1 = the range's end, cut to the window's n
__global__ void __launch_bounds__(256) k_pack_classify_group(PackGroup g, uint32_t p0, uint32_t p1) {
    const uint32_t l = pk_lane_of_rank(g.lanes, blockIdx.y);
    const uint64_t i = (uint64_t)p0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint4* win = (const uint4*)(g.win + (uint64_t)l * g.plane);
    uint32_t tag = 0;
    if (i < p1) {
        const uint4 a = win[2 * i], b = win[2 * i + 1];
        const bool narrow = (a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
        tag = !narrow ? 3u : a.x < 2u ? a.x : 2u;
    }
    const u64 lo = __ballot((tag & 1u) != 0), hi = __ballot((tag >> 1) != 0);
    uint4* planes = (uint4*)(g.pk + (uint64_t)l * g.pk_stride + 32);
    if ((threadIdx.x & 63u) == 0 && i < p1) planes[i >> 6] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__global__ void __launch_bounds__(64) k_pack_scan_chunk_group(PackGroup g, uint32_t nblk, uint32_t nchunk) {
    const uint32_t l = pk_lane_of_rank(g.lanes, blockIdx.y);
    const u64* planes = (const u64*)(g.pk + (uint64_t)l * g.pk_stride + 32);
    const uint32_t lane = threadIdx.x & 63u, b = blockIdx.x * 64 + lane;
    uint32_t c = 0;
    if (b < nblk) { const u64 lo = planes[2 * (uint64_t)b], hi = planes[2 * (uint64_t)b + 1]; c = (uint32_t)__popcll(hi & ~lo) | (uint32_t)__popcll(hi & lo) << 16; }
    uint32_t inc = c;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl(inc, (lane - d) & 63u, 64); if (lane >= d) inc += t; }
    if (b < nblk) g.blk_pre[(uint64_t)l * nblk + b] = inc - c;
    if (lane == 63) g.chunk_tot[(uint64_t)l * nchunk + blockIdx.x] = inc;
}
// one wavefront per selected witness; the header also goes to hdr[rank]: the headers cross PCIe as one piece, ahead of the windows
__global__ void __launch_bounds__(64) k_pack_scan_top_group(PackGroup g, uint64_t first_wire, uint32_t n) {
    const uint32_t l = pk_lane_of_rank(g.lanes, blockIdx.x);
    uint8_t* pk = g.pk + (uint64_t)l * g.pk_stride;
    const uint32_t lane = threadIdx.x & 63u, nblk = (n + 63) / 64, nchunk = (n + 4095) / 4096;
    const uint32_t* chunk_tot = g.chunk_tot + (uint64_t)l * nchunk;
    uint32_t* idx = (uint32_t*)(pk + pk_idx_off(n));
    uint32_t cs = 0, cw = 0;
    for (uint32_t base = 0; base < nchunk; base += 64) {
        const uint32_t c = base + lane, t = c < nchunk ? chunk_tot[c] : 0, s = t & 0xFFFFu, w = t >> 16;
        uint32_t is = s, iw = w;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t ts = __shfl(is, (lane - d) & 63u, 64), tw = __shfl(iw, (lane - d) & 63u, 64);
            if (lane >= d) { is += ts; iw += tw; }
        }
        if (c < nchunk) { idx[2 * (uint64_t)c] = cs + is - s; idx[2 * (uint64_t)c + 1] = cw + iw - w; }
        cs += __shfl(is, 63, 64); cw += __shfl(iw, 63, 64);
    }
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        uint4* hd = (uint4*)g.hdr + 2 * blockIdx.x;
        ((uint4*)pk)[0] = hd[0] = make_uint4(PK_MAGIC, PK_VERSION, (uint32_t)first_wire, (uint32_t)(first_wire >> 32));
        ((uint4*)pk)[1] = hd[1] = make_uint4(n, cs, cw, 0);
    }
    if (lane == 1 && (nblk & 1u)) ((uint4*)(pk + 32))[nblk] = zero;
    const uint32_t ipad = (uint32_t)((pk_pad32(8 * (uint64_t)nchunk) - 8 * (uint64_t)nchunk) / 4);
    if (lane < ipad) idx[2 * (uint64_t)nchunk + lane] = 0;
    const uint32_t spad = (uint32_t)((pk_pad32(4 * (uint64_t)cs) - 4 * (uint64_t)cs) / 4);
    if (lane < spad) ((uint32_t*)(pk + pk_fixed(n)))[(uint64_t)cs + lane] = 0;
}
__global__ void __launch_bounds__(256) k_pack_scatter_group(PackGroup g, uint32_t n, uint32_t p0, uint32_t p1) {
    const uint32_t l = pk_lane_of_rank(g.lanes, blockIdx.y);
    const uint64_t i = (uint64_t)p0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p1) return;
    uint8_t* pk = g.pk + (uint64_t)l * g.pk_stride;
    const uint64_t b = i >> 6; const uint32_t lane = (uint32_t)i & 63u;
    const u64* planes = (const u64*)(pk + 32);
    const u64 lo = planes[2 * b], hi = planes[2 * b + 1];
    if (!((hi >> lane) & 1)) return;
    const uint4* win = (const uint4*)(g.win + (uint64_t)l * g.plane);
    const uint32_t* idx = (const uint32_t*)(pk + pk_idx_off(n));
    const uint32_t pre = g.blk_pre[(uint64_t)l * ((n + 63) / 64) + b];
    const u64 below = ((u64)1 << lane) - 1;
    uint8_t* vals = pk + pk_fixed(n);
    if (!((lo >> lane) & 1)) {
        const uint64_t r = (uint64_t)idx[2 * (i >> 12)] + (pre & 0xFFFFu) + (uint32_t)__popcll(hi & ~lo & below);
        ((uint32_t*)vals)[r] = win[2 * i].x;
    } else {
        const uint32_t n_small = ((const uint32_t*)pk)[5];
        const uint64_t r = (uint64_t)idx[2 * (i >> 12) + 1] + (pre >> 16) + (uint32_t)__popcll(hi & lo & below);
        uint4* dst = (uint4*)(vals + pk_pad32(4 * (uint64_t)n_small)) + 2 * r;
        dst[0] = win[2 * i]; dst[1] = win[2 * i + 1];
    }
}
void launch_group_fill(const PackGroup& g, uint32_t n, bool one_at_0, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, hipStream_t st) {
    const uint32_t nsel = (uint32_t)__builtin_popcountll(g.lanes);
    for (const std::pair<uint32_t, uint32_t>& r : ranges) {
        const uint32_t p0 = r.first * 64, p1 = r.second * 64 < n ? r.second * 64 : n;
        hipLaunchKernelGGL(k_fill_ee_group, dim3((p1 - p0 + 255) / 256, nsel), dim3(256), 0, st, g, p0, p1, one_at_0);
    }
}
void launch_pack_group(const PackGroup& g, uint64_t first_wire, uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, hipStream_t st) {
    const uint32_t nblk = (n + 63) / 64, nchunk = (n + 4095) / 4096, nsel = (uint32_t)__builtin_popcountll(g.lanes);
    for (const std::pair<uint32_t, uint32_t>& r : ranges) {
        const uint32_t p0 = r.first * 64, p1 = r.second * 64 < n ? r.second * 64 : n;
        hipLaunchKernelGGL(k_pack_classify_group, dim3((p1 - p0 + 255) / 256, nsel), dim3(256), 0, st, g, p0, p1);
    }
    hipLaunchKernelGGL(k_pack_scan_chunk_group, dim3(nchunk, nsel), dim3(64), 0, st, g, nblk, nchunk);
    hipLaunchKernelGGL(k_pack_scan_top_group, dim3(nsel), dim3(64), 0, st, g, first_wire, n);
    for (const std::pair<uint32_t, uint32_t>& r : ranges) {
        const uint32_t p0 = r.first * 64, p1 = r.second * 64 < n ? r.second * 64 : n;
        hipLaunchKernelGGL(k_pack_scatter_group, dim3((p1 - p0 + 255) / 256, nsel), dim3(256), 0, st, g, n, p0, p1);
    }
}

// ------------------------------------------------------------------------------------------------ host expansion
namespace {
inline uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline bool all_zero(const uint8_t* p, uint64_t n) { for (uint64_t i = 0; i < n; i++) if (p[i]) return false; return true; }

struct PkView { uint64_t n, ns, nw, nblk, nchunk; const uint8_t *planes, *idx, *small, *wide; };

// everything a reader can recompute is recomputed BEFORE anything is written: length, counts, chunk index and popcounts, padding, and that every value sits under the tag that is its own
bool pk_validate(const uint8_t* pk, uint64_t bytes, PkView& V) {
    if (bytes < 32 || ld32(pk) != PK_MAGIC || ld32(pk + 4) != PK_VERSION || ld32(pk + 28) != 0) return false;
    V.n = ld32(pk + 16); V.ns = ld32(pk + 20); V.nw = ld32(pk + 24);
    if (V.ns + V.nw > V.n) return false;
    V.nblk = (V.n + 63) / 64; V.nchunk = (V.n + 4095) / 4096;
    const uint64_t fixed = pk_fixed(V.n), spad = pk_pad32(4 * V.ns);
    if (bytes != fixed + spad + 32 * V.nw) return false;
    V.planes = pk + 32; V.idx = pk + pk_idx_off(V.n); V.small = pk + fixed; V.wide = V.small + spad;
    uint64_t s = 0, w = 0;
    for (uint64_t b = 0; b < V.nblk; b++) {
        if ((b & 63) == 0 && (ld32(V.idx + 8 * (b >> 6)) != s || ld32(V.idx + 8 * (b >> 6) + 4) != w)) return false;
        const uint64_t lo = ld64(V.planes + 16 * b), hi = ld64(V.planes + 16 * b + 8);
        if (b + 1 == V.nblk && (V.n & 63) && ((lo | hi) & (~0ull << (V.n & 63)))) return false;      // a tag bit beyond n
        s += (uint64_t)__builtin_popcountll(hi & ~lo); w += (uint64_t)__builtin_popcountll(hi & lo);
    }
    if (s != V.ns || w != V.nw) return false;
    if (!all_zero(V.planes + 16 * V.nblk, (size_t)(V.idx - (V.planes + 16 * V.nblk))) || !all_zero(V.idx + 8 * V.nchunk, (size_t)(V.small - (V.idx + 8 * V.nchunk))) ||
        !all_zero(V.small + 4 * V.ns, spad - 4 * V.ns)) return false;
    for (uint64_t k = 0; k < V.ns; k++) if (ld32(V.small + 4 * k) < 2) return false;
    for (uint64_t k = 0; k < V.nw; k++) {
        const uint8_t* v = V.wide + 32 * k;
        if (!(ld32(v + 4) | ld64(v + 8) | ld64(v + 16) | ld64(v + 24))) return false;                 // fits 32 bits: not a wide value
    }
    return true;
}

// chunks [c0, c1): 64 wires from two words; ALIGNED: dst is 16-byte aligned and the stores bypass the cache (nothing of the window is read again by this routine)
template <bool ALIGNED> void pk_expand(const PkView& V, uint8_t* dst, uint64_t c0, uint64_t c1) {
    for (uint64_t c = c0; c < c1; c++) {
        uint64_t s = ld32(V.idx + 8 * c), w = ld32(V.idx + 8 * c + 4);
        const uint64_t b1 = (c + 1) * 64 < V.nblk ? (c + 1) * 64 : V.nblk;
        for (uint64_t b = c * 64; b < b1; b++) {
            const uint64_t lo = ld64(V.planes + 16 * b), hi = ld64(V.planes + 16 * b + 8);
            const uint32_t cnt = (uint32_t)(V.n - 64 * b < 64 ? V.n - 64 * b : 64);
            uint8_t* out = dst + 2048 * b;
#if defined(__SSE2__)
            const __m128i z = _mm_setzero_si128();
            if (hi == 0 && cnt == 64) {                  // the hot loop: nothing but zeros and ones
                for (uint32_t j = 0; j < 64; j++) {
                    const __m128i v = _mm_cvtsi32_si128((int)((lo >> j) & 1));
                    if (ALIGNED) { _mm_stream_si128((__m128i*)(out + 32 * j), v); _mm_stream_si128((__m128i*)(out + 32 * j + 16), z); }
                    else { _mm_storeu_si128((__m128i*)(out + 32 * j), v); _mm_storeu_si128((__m128i*)(out + 32 * j + 16), z); }
                }
                continue;
            }
#endif
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t tag = (uint32_t)((hi >> j) & 1) << 1 | (uint32_t)((lo >> j) & 1);
                if (tag == 3) { memcpy(out + 32 * j, V.wide + 32 * w++, 32); continue; }
                const uint32_t v = tag == 2 ? ld32(V.small + 4 * s++) : tag;
                memset(out + 32 * j, 0, 32); memcpy(out + 32 * j, &v, 4);
            }
        }
    }
#if defined(__SSE2__)
    if (ALIGNED) _mm_sfence();
#endif
}
}  // namespace

extern "C" int pob_unpack_window(const uint8_t* packed, uint64_t packed_bytes, uint8_t* dst, uint64_t dst_cap, int threads) {
    if (!packed || !dst || threads < 0) return POB_E_ARG;
    PkView V;
    if (!pk_validate(packed, packed_bytes, V) || dst_cap < 32 * V.n) return POB_E_ARG;
    if (V.n == 0) return POB_OK;
    const bool aligned = ((uintptr_t)dst & 15) == 0;
    const uint64_t step = 8;                             // chunks per grab: 1 MiB of canonical bytes
    uint32_t nt = threads > 0 ? (uint32_t)threads : pob_pool_width();
    if (nt > (V.nchunk + step - 1) / step) nt = (uint32_t)((V.nchunk + step - 1) / step);
    if (nt == 0) nt = 1;
    std::atomic<uint64_t> next(0);
    const std::function<void(uint32_t)> work = [&](uint32_t) {
        for (;;) {
            const uint64_t c0 = next.fetch_add(step);
            if (c0 >= V.nchunk) return;
            const uint64_t c1 = c0 + step < V.nchunk ? c0 + step : V.nchunk;
            if (aligned) pk_expand<true>(V, dst, c0, c1); else pk_expand<false>(V, dst, c0, c1);
        }
    };
    if (nt == 1) work(0); else pob_pool_run(nt, work);
    return POB_OK;
}
