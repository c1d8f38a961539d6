// The calculator's handle (struct pob_ctx, with the emission's state in EmitState / EmitGroup) and the few host helpers that the host units of libpob_hip.so share:
// pob_host.hip (handle, uploads, generation, evaluation, records, test hooks) and pob_emit.hip (the .wtns emission).  Private: include/pob_hip.h is the interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <array>
#include <functional>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/pob_hip.h"
#include "kernels_common.hpp"
#include "pack_window.hpp"
#include "selfcheck.hpp"

// GROUP EMISSION (pob_emit_begin_group_packed): a payload kind of its own -- the packed windows of every selected witness of one group of 64 from a single pass over the
// resident vector.  d_win: the group's canonical scratch, witness l's window at d_win + l * plane (only the blocks that do not come straight from the Keccak runs are
// ever touched); d_pk[2]: the 64 packed windows (stride pk_stride) of the window being expanded and of the one being copied; h_pin[3]: the selected witnesses' complete
// packed windows, back to back, sized from the fixed parts plus the counts of the headers (h_hdr: those headers, which cross first); the third one is with the caller
struct EmitGroup {
    bool on = false, checked = false; uint32_t group = 0, nsel = 0; uint64_t lanes = 0, alloc_wires = 0, plane = 0, pk_stride = 0, next_bulk = 0;
    uint8_t *d_win = nullptr, *d_pk[2] = {nullptr, nullptr}, *d_hdr[2] = {nullptr, nullptr}, *h_hdr[2] = {nullptr, nullptr}, *h_pin[3] = {nullptr, nullptr, nullptr};
    uint64_t pin_cap[3] = {0, 0, 0}, off[3][64], len[3][64];
    uint32_t *d_blk = nullptr, *d_tot = nullptr;
    hipEvent_t ev_made[2] = {nullptr, nullptr}, ev_hdr[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr}, ev_copied[3] = {nullptr, nullptr, nullptr};
};
// The O0 site tables of a self-check, sorted by wire, on the host (the keys a window is selected by) and on the device (what the kernels read): IsZero words (bit 31:
// child of an IsEqual), M triples {M[k+1], mainInput[k], k} keyed by M[k+1], copy pairs {higher wire, lower wire} keyed by the higher wire.  Two instances: the
// single-witness check's (every recorded site) and the group check's (without the sites inside a Keccak run).  Methods: pob_emit.hip
struct __attribute__((visibility("hidden"))) SiteTables {
    std::vector<uint32_t> z, m_next, c_hi; uint32_t *d_z = nullptr, *d_m = nullptr, *d_c = nullptr;
    struct Range { const uint32_t* p; uint32_t n; };
    struct Window { Range z, m, c; uint64_t total() const { return (uint64_t)z.n + m.n + c.n; } };
    hipError_t upload(const std::vector<std::array<uint32_t, 3>>& ms, const std::vector<std::array<uint32_t, 2>>& cs);     // z is filled by the caller; m_next / c_hi and the device copies from ms / cs
    void free();
    Window window(uint64_t wire_lo, uint64_t wire_hi) const;       // the sites keyed by a wire of [wire_lo, wire_hi), as device ranges
    size_t size() const { return z.size() + m_next.size() + c_hi.size(); }
};
// streaming .wtns emission: two device windows + two pinned host windows, window k+1 is expanded and copied while the caller
// consumes window k (pob_emit_begin / pob_emit_next)
struct EmitState {
    // THREE window slots: one with the caller, one being copied, one being expanded -- so that the first window of the NEXT witness
    // (pob_emit_queue) is expanded while the last windows of the current one are still on their way to the host
    enum { NSLOT = 3 };
    uint8_t* d_win[NSLOT] = {nullptr, nullptr, nullptr}; uint8_t* h_pin[NSLOT] = {nullptr, nullptr, nullptr};
    hipStream_t s_copy = nullptr; hipEvent_t ev_made[NSLOT] = {nullptr, nullptr, nullptr}, ev_copied[NSLOT] = {nullptr, nullptr, nullptr}, ev_free[NSLOT] = {nullptr, nullptr, nullptr};
    uint64_t win_wires = 0, alloc_wires = 0, next_make = 0, next_take = 0, nwin = 0; uint32_t idx = 0; bool active = false;
    uint32_t first_slot = 0;                        // slot of the current witness' window 0 (window k: (first_slot + k) % NSLOT)
    int64_t queued_idx = -1; bool pre_made = false; // pob_emit_queue: the witness the next pob_emit_begin* will ask for / its window 0 is made
    uint64_t pre_made_gen = 0;                       // ... from the resident vector of THIS generation (h->gen_count when the window was expanded)
    std::vector<uint32_t> status_host; uint64_t status_gen = 0;      // the batch's generation statuses, fetched once per generation
    const uint32_t* pin_ptr = nullptr; uint64_t pin_n = 0, pin_id = 0;     // reduced: a map the caller pinned (pob_reduced_map_pin): contents promised unchanged, not hashed again
    struct Run { uint32_t w, b, n, absorb, o, prev, src; };
    std::vector<Run> runs;                          // the Keccak kernels' wires, sorted by wire index: contiguous runs of copies of STORED words (wire index, BIT rank of the source, count) and pieces of Absorb blocks (absorb = 1: stored + alias wires from offset o of the block; b / prev / src = the block's AbsorbRef)
    // which G units write into which window (found by one probe pass per window size): a window launches only those
    uint64_t probe_win = 0, probe_map = 0; uint32_t* d_order = nullptr; unsigned long long* d_probe = nullptr;
    struct WSeg { uint32_t cls, first, count; };
    std::vector<std::vector<WSeg>> wsegs;
    // reduced witness (pob_emit_begin_reduced): the kept O0 wire indices (host copy for the run intersections), their bitmap and the
    // per-word rank on the device; map_id = 0: O0 payload.  total = wires of the payload being emitted (W or the kept count)
    // self-check (pob_emit_selfcheck): site tables (sorted by wire), built once per handle by a recording pass of the emitter; d_sc_res: {lowest violated wire, M sites skipped}
    bool sc_on = false, sc_built = false; SiteTables sc; uint32_t* d_sc_res = nullptr;
    uint64_t sc_checked = 0, sc_skipped = 0;
    // reduced witness: the sites as explicit wire lists, every wire replaced by its class representative (pob_emit_selfcheck_alias) and the sites with a wire that is
    // not kept left out (counted in sc_red_host_skipped); built per map
    std::vector<std::array<uint32_t, 3>> sc_ms; std::vector<std::array<uint32_t, 2>> sc_cs;
    const int32_t* sc_alias = nullptr; uint64_t sc_alias_n = 0, sc_red_map = 0, sc_red_host_skipped = 0; uint32_t sc_red_nz = 0, sc_red_nm = 0;
    uint32_t *d_sc_zr = nullptr, *d_sc_mr = nullptr; std::vector<uint32_t> sc_zr_host, sc_mr_host; bool sc_red_have = false;      // (host copies: pob_debug_selfcheck_sites kinds 3 / 4)
    // group self-check (pob_emit_group_selfcheck), a switch of its own over the same site tables.  gsc_*: the O0 tables without the sites that have a wire inside a Keccak
    // run (gsc_in_runs of them, none expected: the runs' whole blocks never reach the group's scratch); d_gsc_res: 64 verdict words + {skipped, evaluated};
    // gsc_have: a checked group emission has run to its end (the caller has seen n_wires = 0; cleared when the next checked one begins) -- its mask, form and the sites launched
    bool gsc_on = false, gsc_built = false, gsc_have = false, gsc_red = false;
    SiteTables gsc; uint32_t* d_gsc_res = nullptr;
    uint64_t gsc_in_runs = 0, gsc_launched = 0, gsc_lanes = 0;
    // pob_debug_group_emit_xor: armed for the next group emission (xor_armed), in effect during the current one (xor_now)
    struct GXor { uint32_t lane, wire, byte; uint8_t mask; };
    std::vector<GXor> xor_armed, xor_now;
    bool red = false; uint64_t map_id = 0, total = 0; std::vector<uint32_t> keep; unsigned long long* d_rbits = nullptr; uint32_t* d_rpre = nullptr;
    // packed windows (pob_emit_begin_packed, k_pack.hip): part of the payload KIND, like the map.  The pack pass turns the canonical window of a slot into d_pk[slot]; the header,
    // tag planes and chunk index (a length the host knows) are copied with the window, the value sections when the caller takes the window and the header's counts are in
    // pinned memory (s_val: the window copies queued on s_copy wait for expansions that have not run yet).  d_pk_blk / d_pk_tot: the scan's scratch, shared by the slots
    // (every pack pass runs on the handle's own stream).  pk_d2h: bytes the packed emissions of this handle have copied to the host
    bool packed = false, pre_made_packed = false; uint8_t* d_pk[NSLOT] = {nullptr, nullptr, nullptr}; uint32_t *d_pk_blk = nullptr, *d_pk_tot = nullptr; uint64_t pk_alloc_wires = 0, pk_d2h = 0;
    hipStream_t s_val = nullptr;
    EmitGroup grp;                                  // group emission (pob_emit_begin_group_packed)
};

struct pob_ctx {
    int device = 0, circuit = 0;
    Plan plan;
    uint32_t max_batch = 0, groups = 0, n = 0;
    std::string err;
    hipStream_t stream = nullptr;
    // device memory
    uint64_t* d_bits = nullptr; int32_t* d_sm = nullptr; uint32_t* d_fr = nullptr;
    UnitDesc* d_units = nullptr; uint32_t* d_order = nullptr; CircuitLayout* d_L = nullptr;
    SpongeDesc* d_sponges = nullptr; uint32_t *d_perm_sponge = nullptr, *d_perm_block = nullptr;
    uint32_t *d_pos = nullptr, *d_inv = nullptr, *d_pow256 = nullptr; uint32_t npow256 = 0;
    uint32_t* d_emit_ctr = nullptr;                    // EmitP's path counters (pob_debug_emit_counters)
    uint16_t* d_ktab = nullptr;                        // alias table of a KeccakfRound block (keccak_kernels.hpp): which stored wire / constant each of its 102 656 wires is
    // packed inputs, double-buffered: a batch is uploaded into the buffer the current batch does NOT use (generation AND evaluation read the
    // inputs), pob_generate switches; ev_in_done[b] = the last generation / evaluation that read buffer b
    uint8_t* d_in_fr[2] = {nullptr, nullptr}; int32_t* d_in_sm[2] = {nullptr, nullptr}; int in_cur = 0, in_next = 0; uint32_t n_next = 0;
    hipEvent_t ev_in_done[2] = {nullptr, nullptr}; bool in_done_rec[2] = {false, false};
    uint8_t* d_in_sm8[2] = {nullptr, nullptr}; pob_sm_exc_t* d_in_exc[2] = {nullptr, nullptr};      // staging of the byte form (pob_upload_inputs8*): 11 KB per witness and buffer
    bool in_bytes[2] = {false, false};                  // buffer b holds its batch in the byte form only (ProofOfBurn: the inputs' wires are written straight from it, k_inputs8; d_in_sm[b] is stale)
    uint32_t *d_status_raw = nullptr, *d_status = nullptr, *d_chk = nullptr, *d_bad = nullptr, *d_records = nullptr; uint8_t* d_outputs = nullptr;
    EmitState em;                                      // the emission's state (pob_emit.hip)
    // schedule
    std::vector<uint32_t> order;                       // unit indices grouped by (stage, lds flag)
    struct Seg { uint32_t stage, lds, first, count; };
    std::vector<Seg> segs, emit_segs, chk_segs;        // per (stage, class) for generation; per class for emission; per FAMILY for evaluation
    hipStream_t stream2 = nullptr, stream3 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join3 = nullptr;
    struct KSeg { uint32_t stage, sp_first, sp_count, perm_first, perm_count; hipEvent_t ev_done; };
    std::vector<KSeg> ksegs;                           // ev_done: recorded behind the segment's sponge kernels in pob_generate
    hipStream_t stream_k = nullptr;                                     // the main track's round expansion in pipeline mode (pob_generate)
    hipEvent_t ev_rounds_fork = nullptr, ev_g_done = nullptr, ev_k_done = nullptr;   // pipeline: the G side of a generation is enqueued / the Keccak evaluation on the streaming stream is done
    // side tracks (Plan::track_fork/track_join): streams of the device's pool (StreamPool below), own fork/join events, start and end events
    // (ROCm multiplexes streams onto few hardware queues: a lone handle keeps to the caller's stream + 4 of the pool's --
    //  stream2, track 1's (also track 6), track 2's (also track 3, which runs before it anyway), the round expansion's; a track's BN254 and light
    //  launches of one stage share its stream)
    struct Track { hipStream_t s_main = nullptr, s_heavy = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_start = nullptr, ev_end = nullptr; };
    Track tracks[Plan::MAX_TRACKS];
    uint32_t nperms = 0;
    // IN-ORDER schedule (pob_set_inorder): the whole generation / evaluation of the calculator on the CALLER's stream, no side stream and no event; a job gets
    // its concurrency from keeping several such calculators in flight, each on a stream of its own.  The stage graph is flattened into LEVELS (longest
    // dependency path): every unit of a level, of whatever track, goes out in one launch per kernel class, then the level's sponges; the round expansion of
    // every sponge is ONE launch at the end (nothing of the generation reads it).
    bool inorder = false;
    // FUSED launch (pob_set_inorder(h, 3), what bench.py runs): the lane-spread Poseidon blocks share a launch with the sponge chain that does not depend on them (header and
    // layers: the longest chain) -- two launches of a few hundred wavefronts each, both a long serial chain per wavefront, neither near any throughput limit: side by side
    // they take the longer one's time.  gen_plan[0]: one launch per kernel (round 5), [1]: with the fused launch.
    // (Round 6 also fused the bandwidth-bound kernels with latency-bound ones -- slices of the round expansion with the levels behind the chain, the round evaluation
    //  interleaved with the wide evaluation families, the chain evaluation behind the narrow families: such a launch lasts about the SUM of its parts (a latency-bound
    //  wavefront makes next to no progress while the memory system is saturated), the loop did not move; removed.  profiles/round6_experiments.txt)
    bool fused = false;
    // EVALUATION THAT RIDES WITH THE GENERATION (pob_set_inorder bit 2): the generation's last launch is k_rounds_gc -- every round block is evaluated by the wavefront that has
    // just written it, its loads served by L2 -- and the input rows are compared with the inputs by the launch that writes them (k_inputs MODE 2); the evaluation that follows
    // skips those two kernels.  rode: the resident vector is the one those launches evaluated (cleared by every debug poke: the evaluation then runs k_rounds_check and the
    // input check over the vector as it is)
    bool gc = false, rode = false;
    // ... and so does the evaluation of everything else but the sponge chains (the two main circuits: every G unit's stores are loaded back and compared, policy.hpp GenPT<true>,
    // poseidon_wide.hpp PosWideT<true>): pob_constraint_check then runs k_chain_check and collects the records
    bool rode_g = false;
    bool fault_armed = false, fault_g = false; int fault_cls = 0; uint32_t fault_group = 0; uint64_t fault_word = 0, fault_mask = 0;     // pob_debug_store_fault (tests)
    bool fault_value = false;                             // ... armed by pob_debug_value_fault: the unit goes on with the corrupted value (FAULT_VALUE)
    // AUDIT (pob_set_audit): every audit_period-th pob_constraint_check whose launches were skipped because the generation rode runs them after all for a window of
    // audit_groups consecutive groups from audit_cursor -- the independent evaluation of a riding calculator.  audit_tick: checks since pob_set_audit;
    // audit_first / audit_n: what the last check evaluated (pob_audit_last)
    uint32_t audit_groups = 0, audit_period = 1, audit_cursor = 0, audit_first = 0, audit_n = 0; uint64_t audit_tick = 0, audit_batches = 0, audit_group_total = 0;
    struct GenLaunch { uint32_t kind, cls, first, count, k_first, k_count; };
    enum { GL_UNITS = 0, GL_CHAIN = 1, GL_POS_CHAIN = 2, GL_ROUNDS = 4 };
    std::vector<GenLaunch> gen_plan[2];
    Seg chk_narrow{0, 0, 0, 0};                          // in-order evaluation: the units of the four narrow families, one launch
    Seg chk_ride_kept{0, F_RL, 0, 0};                    // ... when the G units' evaluation rode with their generation: the units whose generation did not ride (circuits.hpp ride_keeps_evaluation)
    uint32_t nlevels = 0;
    bool generated = false; uint64_t gen_count = 0;
    // two-batch pipeline (pob_set_partner): this handle's generation starts with the partner's evaluation and its Keccak expansion
    // waits for the end of that evaluation; the evaluation then uses the pool's two evaluation streams
    pob_ctx* partner = nullptr; struct StreamPool* pool = nullptr;
    hipEvent_t ev_gen_done = nullptr, ev_check_done = nullptr; bool gen_done_rec = false, check_done_rec = false, evaluated = false;
    hipStream_t gen_stream = nullptr, chk_stream = nullptr; bool gen_ordered = false, chk_ordered = false;      // where the last generation / evaluation was enqueued (a call on ANOTHER stream is ordered behind it by its event)
    // service loop: asynchronous input upload (own stream, pob_upload_inputs_async) and per-batch result records into pinned memory
    hipStream_t s_upload = nullptr;                         // = the pool's upload stream
    hipEvent_t ev_upload = nullptr, ev_rec[2] = {nullptr, nullptr};   // ev_rec[s]: the records of buffer s are written
    // timing events around the Keccak round evaluation (pob_probe_check_kernel): one pair per record slot -- the kernel of the batch whose records sit in slot s -- because the
    // evaluation that rides with the expansion records them in pob_generate, and the caller reads the previous batch's pair after it has enqueued the next generation
    bool kchk_rec[2] = {false, false}; hipEvent_t ev_kchk[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint8_t* h_records[2] = {nullptr, nullptr}; int rec_slot = 0, fetch_slot = 0; uint32_t rec_n[2] = {0, 0}; bool upload_pending = false, have_next = false, fetch_pending = false;
};

#define HIPC(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return POB_E_HIP; } } while (0)

// The emission's six small kernels are DEFINED in pob_host.hip and launched from pob_emit.hip: a unit's device code is compiled as one module, and in a module of their own
// these kernels came out with another register assignment around their calls of fr_mul (65 / 67 VGPRs for 66 / 68, the same instructions) -- where they are, the
// library's device code is the parent's bit for bit.  Their descriptions are with their definitions.
__global__ void k_selfcheck_z(ScWin W, const uint32_t* sites, uint32_t n, uint32_t* res);
__global__ void k_selfcheck_c(ScWin W, const uint32_t* sites, uint32_t n, uint32_t* res);
__global__ void k_selfcheck_m(ScWin W, const uint32_t* sites, uint32_t n, const uint32_t* pow256, uint32_t* res);
__global__ void k_selfcheck_zr(ScWin W, const uint32_t* zw, uint32_t n, uint32_t* res);
__global__ void k_selfcheck_mr(ScWin W, const uint32_t* mw, uint32_t n, const uint32_t* pow256, uint32_t* res);
__global__ void k_fill_ee(uint4* p, uint64_t n16);

// host helpers of pob_host.hip that the emission uses too (not part of the C ABI: hidden)
namespace pob_detail __attribute__((visibility("hidden"))) {
hipStream_t own_stream(pob_ctx* h);      // the handle's own stream (callers that pass no stream, emission, test hooks): created on first use
GArgs gargs(pob_ctx* h);
void launch_g_emit(const GArgs& A, uint32_t cls, uint32_t nunits, hipStream_t st);
void launch_g_emit_group(const GArgs& A, uint32_t cls, uint32_t nunits, hipStream_t st);
void emit_release(pob_ctx* h);           // pob_close: the emission's buffers and events (before the device is idle) ...
void emit_release_streams(pob_ctx* h);   // ... and its two streams (after)
}
using namespace pob_detail;
