// Group emission, the Keccak runs' side (pob_emit_begin_group_packed): every selected witness of a group of 64 from ONE pass over the resident BIT slab.
//
// The resident layout of a BIT wire is one 64-bit word, bit l = its value in witness l.  For 64 consecutive wires the 64 x 64 bit matrix of their words is, row-wise per
// witness, exactly the `lo` tag word of that block of the packed format (k_pack.hip), and `hi` is 0 -- a BIT wire is 0 or 1.  k_emit_group_direct loads the words lane = wire,
// transposes them across the wavefront (DevPol::xpose64: six butterfly stages) and stores witness l's word into witness l's tag plane: the canonical 32-byte form of
// these wires (97.5 % of an O0 witness) is never written.  Blocks only partly inside a run, and the whole reduced form (kept wires land at their ranks), go through
// k_emit_group_canon into the group's canonical scratch, like the wires of the G units.
#include "keccak_kernels.hpp"

// the 64-witness word of wire t of the run: a stored word (tab == nullptr: BIT rank base + t) or offset base + t of an Absorb block, negation applied
__device__ __forceinline__ u64 group_run_word(const u64* G, const AbsorbRef ab, uint32_t base, uint32_t t, const uint16_t* tab) {
    if (!tab) return G[base + t];
    uint32_t neg;
    const u64 word = absorb_wire_word(G, ab, base + t, tab, &neg);
    return neg ? ~word : word;
}

// one wavefront = GD_BLOCKS consecutive 64-wire blocks: lane l leaves with GD_BLOCKS {lo, hi = 0} pairs of its witness, one contiguous 128-byte piece of its tag plane
#define GD_BLOCKS 8
__global__ void __launch_bounds__(64) k_emit_group_direct(const u64* G, uint8_t* pk, uint64_t pk_stride, uint64_t lanes, uint32_t blk0, uint32_t nblk, AbsorbRef ab,
                                                          uint32_t base, const uint16_t* tab) {
    const uint32_t lane = threadIdx.x & 63u, b0 = blockIdx.x * GD_BLOCKS;
    DevPol p; p.m.lane = lane;
    u64 lo[GD_BLOCKS];
#pragma unroll
    for (uint32_t j = 0; j < GD_BLOCKS; j++) {
        const u64 word = b0 + j < nblk ? group_run_word(G, ab, base, 64u * (b0 + j) + lane, tab) : 0;       // lane = wire ...
        lo[j] = p.xpose(word, 64);                                                                          // ... lane = witness
    }
    if (!((lanes >> lane) & 1)) return;
    uint4* dst = (uint4*)(pk + (uint64_t)lane * pk_stride + 32) + blk0 + b0;
#pragma unroll
    for (uint32_t j = 0; j < GD_BLOCKS; j++) if (b0 + j < nblk) dst[j] = make_uint4((uint32_t)lo[j], (uint32_t)(lo[j] >> 32), 0, 0);
}

// canonical route: thread = wire, the word is loaded once and its 64 bits go to the 64 witnesses' windows (for one witness the threads of a wavefront write one contiguous 2 KB piece)
__global__ void __launch_bounds__(256) k_emit_group_canon(const u64* G, GroupWin W, uint32_t wire0, AbsorbRef ab, uint32_t base, uint32_t count, const uint16_t* tab) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
        uint32_t p = wire0 + t;
        if (W.rbits) {
            const unsigned long long word_k = W.rbits[p >> 6];
            if (!((word_k >> (p & 63)) & 1)) continue;
            p = W.rpre[p >> 6] + (uint32_t)__popcll(word_k & ((1ull << (p & 63)) - 1));
        }
        p -= W.k0;
        if (p >= W.kn) continue;
        const u64 word = group_run_word(G, ab, base, t, tab);
        uint8_t* q = W.win + (uint64_t)p * 32;
        for (uint64_t ls = W.lanes; ls; ls &= ls - 1) {
            const uint32_t l = (uint32_t)__builtin_ctzll(ls);
            uint4* d = (uint4*)(q + (uint64_t)l * W.plane);
            d[0] = make_uint4((uint32_t)((word >> l) & 1), 0, 0, 0); d[1] = make_uint4(0, 0, 0, 0);
        }
    }
}

void launch_k_emit_group_canon(const u64* G, GroupWin W, uint32_t wire0, AbsorbRef B, uint32_t o0_or_bit_base, uint32_t count, const uint16_t* tab, hipStream_t st) {
    uint32_t blocks = (count + 255) / 256; if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_emit_group_canon, dim3(blocks), dim3(256), 0, st, G, W, wire0, B, o0_or_bit_base, count, tab);
}
void launch_k_emit_group_direct(const u64* G, uint8_t* pk, uint64_t pk_stride, uint64_t lanes, uint32_t blk0, uint32_t nblk, AbsorbRef B, uint32_t o0_or_bit_base,
                                const uint16_t* tab, hipStream_t st) {
    hipLaunchKernelGGL(k_emit_group_direct, dim3((nblk + GD_BLOCKS - 1) / GD_BLOCKS), dim3(64), 0, st, G, pk, pk_stride, lanes, blk0, nblk, B, o0_or_bit_base, tab);
}
