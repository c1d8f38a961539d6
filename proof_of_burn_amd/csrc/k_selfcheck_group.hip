// Self-check of a GROUP emission (pob_emit_group_selfcheck): the relations of the derived wires (selfcheck.hpp: the statements the single-witness kernels evaluate) on the
// values the group emitter wrote into each selected witness' window of the canonical scratch, behind the scratch's last writer and in front of the pack pass.
// lane = site, blockIdx.y = rank of the witness among the selected lanes: the sites are sorted by wire, so neighbouring lanes read neighbouring 32-byte values of ONE
// witness' plane (lane = witness would stride by the plane, 128 MiB at the default window).  A wavefront reduces before it touches memory: at most one atomicMin reaches
// the witness' verdict word, and only the blockIdx.y == 0 slice counts the skipped / evaluated sites (they depend on positions, not on values: the counts are per witness
// and the same for every selected one), with one atomicAdd of the wavefront's popcount per counter.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "selfcheck.hpp"

__device__ __forceinline__ uint32_t scg_lane_of_rank(u64 lanes, uint32_t r) { for (uint32_t k = 0; k < r; k++) lanes &= lanes - 1; return (uint32_t)__builtin_ctzll(lanes); }
__device__ __forceinline__ ScWin scg_window(const ScGroup& G, uint32_t l) { return ScWin{G.win + (uint64_t)l * G.plane, G.w0, G.wn, G.rbits, G.rpre}; }
// every lane of the wavefront arrives here (a lane beyond the sites with r = SC_NONE)
__device__ __forceinline__ void scg_finish(const ScGroup& G, uint32_t l, uint32_t r, uint32_t wire) {
    const uint32_t lane = threadIdx.x & 63u;
    if (__ballot(r == SC_BAD)) {
        uint32_t v = r == SC_BAD ? wire : 0xFFFFFFFFu;
        for (int m = 32; m; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor(v, m, 64); v = o < v ? o : v; }
        if (lane == 0) atomicMin(G.bad + l, v);
    }
    if (blockIdx.y == 0) {
        const u64 sk = __ballot(r == SC_SKIP), ev = __ballot(r == SC_OK || r == SC_BAD);
        if (lane == 0) {
            if (sk) atomicAdd(G.cnt, (uint32_t)__popcll(sk));
            if (ev) atomicAdd(G.cnt + 1, (uint32_t)__popcll(ev));
        }
    }
}

__global__ void __launch_bounds__(64) k_selfcheck_group_z(ScGroup G, const uint32_t* sites, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = scg_lane_of_rank(G.lanes, blockIdx.y);
    uint32_t r = SC_NONE, wire = 0xFFFFFFFFu;
    if (t < n) r = sc_rel_z(scg_window(G, l), sites[t], &wire);
    scg_finish(G, l, r, wire);
}
__global__ void __launch_bounds__(64) k_selfcheck_group_c(ScGroup G, const uint32_t* sites, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = scg_lane_of_rank(G.lanes, blockIdx.y);
    uint32_t r = SC_NONE, wire = 0xFFFFFFFFu;
    if (t < n) r = sc_rel_c(scg_window(G, l), sites[2 * (size_t)t], sites[2 * (size_t)t + 1], &wire);
    scg_finish(G, l, r, wire);
}
__global__ void __launch_bounds__(64) k_selfcheck_group_m(ScGroup G, const uint32_t* sites, uint32_t n, const uint32_t* pow256) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = scg_lane_of_rank(G.lanes, blockIdx.y);
    uint32_t r = SC_NONE, wire = 0xFFFFFFFFu;
    if (t < n) r = sc_rel_m(scg_window(G, l), sites[3 * (size_t)t], sites[3 * (size_t)t + 1], sites[3 * (size_t)t + 2], pow256, &wire);
    scg_finish(G, l, r, wire);
}
__global__ void __launch_bounds__(64) k_selfcheck_group_zr(ScGroup G, const uint32_t* zw, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = scg_lane_of_rank(G.lanes, blockIdx.y);
    uint32_t r = SC_NONE, wire = 0xFFFFFFFFu;
    if (t < n) r = sc_rel_zr(scg_window(G, l), zw + 6 * (size_t)t, &wire);
    scg_finish(G, l, r, wire);
}
__global__ void __launch_bounds__(64) k_selfcheck_group_mr(ScGroup G, const uint32_t* mw, uint32_t n, const uint32_t* pow256) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, l = scg_lane_of_rank(G.lanes, blockIdx.y);
    uint32_t r = SC_NONE, wire = 0xFFFFFFFFu;
    if (t < n) r = sc_rel_mr(scg_window(G, l), mw + 4 * (size_t)t, pow256, &wire);
    scg_finish(G, l, r, wire);
}
__global__ void k_group_xor_byte(uint8_t* p, uint8_t mask) { *p ^= mask; }

// (plain locals in front of the launches: the CPU shim's launch macro evaluates its arguments inside a by-copy lambda)
static uint32_t scg_nsel(const ScGroup& G) { return (uint32_t)__builtin_popcountll(G.lanes); }
void launch_selfcheck_group_z(const ScGroup& G, const uint32_t* sites, uint32_t n, hipStream_t st) {
    const ScGroup g = G;
    if (n && g.lanes) hipLaunchKernelGGL(k_selfcheck_group_z, dim3((n + 63) / 64, scg_nsel(g)), dim3(64), 0, st, g, sites, n);
}
void launch_selfcheck_group_c(const ScGroup& G, const uint32_t* sites, uint32_t n, hipStream_t st) {
    const ScGroup g = G;
    if (n && g.lanes) hipLaunchKernelGGL(k_selfcheck_group_c, dim3((n + 63) / 64, scg_nsel(g)), dim3(64), 0, st, g, sites, n);
}
void launch_selfcheck_group_m(const ScGroup& G, const uint32_t* sites, uint32_t n, const uint32_t* pow256, hipStream_t st) {
    const ScGroup g = G;
    if (n && g.lanes) hipLaunchKernelGGL(k_selfcheck_group_m, dim3((n + 63) / 64, scg_nsel(g)), dim3(64), 0, st, g, sites, n, pow256);
}
void launch_selfcheck_group_zr(const ScGroup& G, const uint32_t* zw, uint32_t n, hipStream_t st) {
    const ScGroup g = G;
    if (n && g.lanes) hipLaunchKernelGGL(k_selfcheck_group_zr, dim3((n + 63) / 64, scg_nsel(g)), dim3(64), 0, st, g, zw, n);
}
void launch_selfcheck_group_mr(const ScGroup& G, const uint32_t* mw, uint32_t n, const uint32_t* pow256, hipStream_t st) {
    const ScGroup g = G;
    if (n && g.lanes) hipLaunchKernelGGL(k_selfcheck_group_mr, dim3((n + 63) / 64, scg_nsel(g)), dim3(64), 0, st, g, mw, n, pow256);
}
void launch_group_xor_byte(uint8_t* p, uint8_t mask, hipStream_t st) { hipLaunchKernelGGL(k_group_xor_byte, dim3(1), dim3(1), 0, st, p, mask); }
