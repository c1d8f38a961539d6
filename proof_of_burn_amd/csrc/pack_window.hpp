// Packed emission windows (k_pack.hip) and the loader's thread pool (pack_json.hip), for the host scheduler (pob_host.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <utility>
#include <vector>

// the canonical window win[n][32] of payload positions first_wire .. -> the packed form at pk (pack_fixed_bytes(n) + 32 * n + 32 bytes hold any window of n wires);
// blk_pre[ceil(n / 64)] and chunk_tot[ceil(n / 4096)] are scratch.  The header, the tag planes and the chunk index are the first pack_fixed_bytes(n) bytes;
// pack_value_bytes(n_small, n_wide) bytes of values follow, with the two counts taken from the header
void launch_pack_window(const uint8_t* win, uint64_t first_wire, uint32_t n, uint8_t* pk, uint32_t* blk_pre, uint32_t* chunk_tot, hipStream_t st);
// group emission: the same pass over the 64 canonical windows of a group (witness l: win + l * plane -> pk + l * pk_stride; bit l of lanes = witness l is emitted, nothing is
// launched for the others).  ranges: the 64-position block ranges [b0, b1) of the window that HAVE a canonical form, in order; the blocks between them hold their plane words
// already (hi = 0) and are read by the scan only.  blk_pre[64][ceil(n / 64)], chunk_tot[64][ceil(n / 4096)]: scratch; hdr: popcount(lanes) x 32 B, the selected witnesses'
// headers in lane order.  launch_group_fill: 0xEE.. into the ranges (one_at_0: 1 at position 0)
struct PackGroup { uint8_t* win; uint64_t plane; uint8_t* pk; uint64_t pk_stride, lanes; uint32_t *blk_pre, *chunk_tot; uint8_t* hdr; };
void launch_group_fill(const PackGroup& g, uint32_t n, bool one_at_0, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, hipStream_t st);
void launch_pack_group(const PackGroup& g, uint64_t first_wire, uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, hipStream_t st);
uint64_t pack_fixed_bytes(uint64_t n);
uint64_t pack_value_bytes(uint64_t n_small, uint64_t n_wide);
// the loader's persistent pool: fn(0) on the caller and fn(1 .. threads - 1) on pool threads, back when all are done; its default width
void pob_pool_run(uint32_t threads, const std::function<void(uint32_t)>& fn);
uint32_t pob_pool_width();
