// Poseidon(T-1) generation with the STATE spread over lanes (circomlib poseidon.circom, optimised schedule; the block layout is
// the one gadgets.hpp gPoseidon walks: reference circuits/proof_of_burn.circom:113-119, utils/burn_address.circom:55-57,
// spend.circom:43-44 are the call sites).
//
// The lane = witness form (gadgets.hpp) runs a Poseidon block as ONE dependent chain of 600-1 040 Montgomery products per
// wavefront, 16 wavefronts per batch of 1 024: 1.1-1.7 ms alone and 3-5 ms beside a streaming kernel.  Here a wavefront holds
// 16 witnesses x 4 lanes (lane = 4 * witness + j): lane j holds element j, and for T = 5 lane 1 holds element 4 as well;
//   * full round: the S-boxes of a witness are three products deep (x^2, x^4, x^5; six on the two-element lane); Mix is T products
//     per element with the round's inputs broadcast inside the 4-lane group (ds_bpermute);
//   * partial round: lane 0 runs the S-box while lanes 1.. multiply their MixS coefficients into their elements in the same four
//     product slots (table at the partial-round loop), then a 2-step sum over the group: 4 products deep instead of 3 + (2T - 1);
// critical path 360 products instead of 1 040 for T = 5 (280 / 784 for T = 4, 276 / 600 for T = 3).  Round 6's 8 lanes per witness
// (304 for T = 5) left lanes T..7 idle and ran all four products of a partial round on every lane: twice the multiplier work.
// The HBM layout is untouched (limb planes [wire][limb][64 witnesses]): a lane stores its elements' wires for its witness, the
// 16 witnesses of a wave are 64 contiguous bytes of a row.  Evaluation (CK_POS_SEG units) and emission keep the lane = witness code.
//
// Generation only.  One wavefront = (unit, group, 16-witness slice); a workgroup = POSW_WAVES wavefronts = consecutive slices of ONE unit, which share one copy of the
// constants of the unit's T in LDS (22 KB for T = 5: with a copy per wavefront -- round 5 -- the LDS held five wavefronts per CU, and beside other calculators' Poseidon
// blocks that occupancy, not the multiplier, bounded the launch).
#pragma once
#include "kernels_common.hpp"

extern __shared__ uint32_t g_lds[];

// which wires feed the block (FR ranks; POSW_NONE = absent).  Input 0 is always POSEIDON_PREFIX + pre (constants.circom:3-14).
#define POSW_NONE 0xFFFFFFFFu

// STORE SLOTS.  A block's words go to memory in slots: in one slot every lane of a witness's 4-lane group stores ONE word of its own choice -- (on, FR rank, value) per lane, so a
// word may leave from a lane that does not hold its element: lane 0's S-box words of a partial round and element 4's words (T = 5, lane 1) ride on the lanes that would idle,
// moved inside the quad (posw_quad).  A partial round is ceil(words / 4) slots (4 / 3 / 3 for T = 5 / 4 / 3; for T = 3 the fourth lane carries words though it holds no element),
// a T = 5 full round 11 (8 for each lane's own element + 3 for element 4's eight words; 16 before), the head 5 / 4 (9 / 5), the tail 8 / 6 (14 / 9).  The words where the block goes on with what the store
// returns (posw_value_fault_covers) never move: they stay on the lane that holds the element.
//
// RIDE (in-order calculators, pob_set_inorder bit 2): the evaluation rides with the generation as in policy.hpp GenPT<true> -- every word a lane stores is loaded back and
// compared with the value stored; a mismatch marks the word's wire (the lowest per lane; poswide_body reduces over the 4 lanes of a witness).  With it the Poseidon segments of
// pob_constraint_check (CK_POS_SEG: the stored states recomputed from stored operands) need not run.  The load-backs go by batches of up to POSW_RING slots: put<I>() stores
// slot I and keeps (value, offset), back<N>() issues the N slots' loads behind all their stores, resolve<N>() compares them -- placed behind the NEXT products (a partial
// round's batch resolves behind the next round's first product), so that no store waits for the load of the store before it.
#define POSW_OFF 0xFFFFF000u       // a slot's offset on a lane that stores nothing: past the slab, the store is dropped
#define POSW_RING 4
template <bool RIDE, bool FAULT = false> struct PosWideT {
    __amdgpu_buffer_rsrc_t rs;     // the group's FR slab
    uint32_t slot4;                // witness slot (0..63) * 4
    bool act;                      // this lane's state slot is in use (element j < T)
    bool actb;                     // ... and it holds a second one, element 4 (T = 5, lane 1)
    const uint32_t* ktab;          // Poseidon table of this T in LDS, indexed from the first constant of T
    uint32_t kbase;                // table index of that first constant
    uint32_t w_of_f;               // wire index of FR rank f inside the block = f + w_of_f (the block's wires are all field elements, in rank order)
    uint32_t w_also;               // ... of the caller's copy of the hash (outside the block): reported at the block's first wire
    mutable Fr pl[POSW_RING], pv[POSW_RING]; mutable uint32_t po[POSW_RING], bad;      // RIDE: the pending slots (loaded, stored, offset = (rank << 11) + slot4 or POSW_OFF) and the lowest wire that differed
    uint32_t fault_f; bool fault_me;                  // FAULT (tests, pob_debug_store_fault): FR rank whose store reaches memory with bit 0 flipped, for this lane's witness
    bool fault_val;                                   // ... pob_debug_value_fault: the element is wrong BEFORE the store -- the load-back agrees, put() returns it and the block goes on with it
                                                      //     where the stored element is the running state (posw_value_fault_covers)
    __device__ __forceinline__ void ride_init() {
#pragma unroll
        for (int i = 0; i < POSW_RING; i++) { pl[i] = pv[i] = fr_zero(); po[i] = POSW_OFF; }
        bad = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ Fr ld(uint32_t f) const {
        Fr v; const uint32_t off = act ? (f << 11) + slot4 : POSW_OFF;          // inactive: past the slab, reads 0
#pragma unroll
        for (int k = 0; k < 8; k++) v.l[k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + 256u * k), 0, 0);
        return v;
    }
    // the element the block goes on with: v (FAULT, a value fault armed on this element: v with bit 0 flipped).  put() applies it; a lane that needs the element
    // before its slot leaves calls vf() itself and passes pre = true to put()
    __device__ __forceinline__ Fr vf(bool on, uint32_t f, const Fr& v_in) const {
        Fr v = v_in;
        if constexpr (FAULT) { if (fault_val && fault_me && on && f == fault_f) v.l[0] ^= 1u; }
        return v;
    }
    // slot I of the batch: this lane's word (on: it has one; f: its FR rank) -> the element the block goes on with
    template <int I> __device__ __forceinline__ Fr put(bool on, uint32_t f, const Fr& v_in, bool pre = false) const {
        static_assert(I >= 0 && I < POSW_RING, "slot index");
        const uint32_t off = on ? (f << 11) + slot4 : POSW_OFF;
        Fr v = v_in;
        if constexpr (FAULT) { if (!pre) v = vf(on, f, v_in); }
        const uint32_t flip = (FAULT && !fault_val && fault_me && f == fault_f) ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) __builtin_amdgcn_raw_buffer_store_b32((int)(k == 0 ? v.l[0] ^ flip : v.l[k]), rs, (int)(off + 256u * k), 0, 0);
        if constexpr (RIDE) { pv[I] = v; po[I] = off; }
        return v;
    }
    // the load-backs of slots 0..N-1, behind all their stores (the offset is opaque: the stored value cannot be forwarded)
    template <int N> __device__ __forceinline__ void back() const {
        if constexpr (RIDE) {
#pragma unroll
            for (int i = 0; i < N; i++) {
                uint32_t off = po[i]; POB_OPAQUE(off);                          // (a lane without a word: past the slab, reads 0; not compared)
#pragma unroll
                for (int k = 0; k < 8; k++) pl[i].l[k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + 256u * k), 0, 0);
            }
            POB_RIDE_BARRIER();
        }
    }
    // compares slots 0..N-1 with what was stored (al: this lane's word in slot ALSO is the caller's copy of the hash)
    template <int N, int ALSO = -1> __device__ __forceinline__ void resolve(bool al = false) const {
        if constexpr (RIDE) {
            POB_RIDE_BARRIER();
#pragma unroll
            for (int i = 0; i < N; i++) {
                uint32_t w = (po[i] >> 11) + w_of_f;
                if (i == ALSO && al) w = w_also;
                if (po[i] != POSW_OFF && !fr_eq(pl[i], pv[i]) && w < bad) bad = w;
            }
            POB_OPAQUE(bad);
        }
    }
    // slots FROM.. hold nothing: a round begins with resolve<POSW_RING>() whatever the batch before it was
    template <int FROM> __device__ __forceinline__ void idle() const {
        if constexpr (RIDE) {
#pragma unroll
            for (int i = FROM; i < POSW_RING; i++) po[i] = POSW_OFF;
        }
    }
    __device__ __forceinline__ Fr kc(uint32_t idx) const {                      // table constant (per-lane index)
        Fr v; const uint32_t* q = ktab + (size_t)(idx - kbase) * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) v.l[k] = q[k];
        return v;
    }
};
typedef PosWideT<false> PosWide;
__device__ __forceinline__ Fr posw_from(const Fr& v, uint32_t src_lane) {      // every lane := lane src_lane's element
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v.l[k]);
    return r;
}
// every lane := the element of lane Q of its 4-lane group (g0 = the group's first lane): a DPP quad permute on the device, one VALU move per limb and no LDS traffic;
// the shim has no DPP and takes the same value through its bpermute
template <int Q> __device__ __forceinline__ Fr posw_quad(const Fr& v, uint32_t g0) {
#ifdef POB_HOSTSIM
    return posw_from(v, g0 | (uint32_t)Q);
#else
    Fr r; (void)g0;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.l[k], Q * 0x55, 0xF, 0xF, true);     // quad_perm:[Q,Q,Q,Q]
    return r;
#endif
}
// lane j of a group takes its own one of four (a slot's per-lane rank / value)
__device__ __forceinline__ uint32_t posw_pick(uint32_t j, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return j < 2 ? (j == 0 ? a : b) : (j == 2 ? c : d); }
__device__ __forceinline__ Fr posw_pick(uint32_t j, const Fr& a, const Fr& b, const Fr& c, const Fr& d) { return fr_sel(j < 2, fr_sel(j == 0, a, b), fr_sel(j == 2, c, d)); }
__device__ __forceinline__ Fr posw_group_sum(Fr v, uint32_t lane) {            // sum over the 4 lanes of a witness, in every lane
#pragma unroll
    for (uint32_t m = 2; m >= 1; m >>= 1) v = fr_add(v, posw_from(v, lane ^ m));
    return v;
}

// the unit's descriptor as scalars (read through the scalar cache: the unit index is wave-uniform)
struct PosWDesc { uint32_t base, pre, in2, in3, in4, sub, also; };
// the block's element e (< T) on entry: inputs[e-1] (element 1: POSEIDON_PREFIX + pre; the last one minus d.sub), element 0 = 0
template <int T, class PW> __device__ __forceinline__ Fr posw_input(const GArgs& A, const PosWDesc& d, const PW& W, uint32_t e, bool act) {
    Fr x = fr_zero();
    if (e == 1) x = A.L->prefix[d.pre];
    uint32_t a2 = e == 2 ? d.in2 : 0u, a3 = e == 3 ? d.in3 : 0u, a4 = e == 4 ? d.in4 : 0u;
    POB_OPAQUE(a2); POB_OPAQUE(a3); POB_OPAQUE(a4);               // (left alone, the selects become a dynamically indexed table in scratch)
    const uint32_t aj = a2 | a3 | a4;
    const uint32_t src = (act && e >= 2) ? aj : POSW_NONE;
    PosWideT<false> Wi; Wi.rs = W.rs; Wi.slot4 = W.slot4; Wi.act = src != POSW_NONE;
    const Fr v = Wi.ld(src);
    if (src != POSW_NONE) x = v;
    const uint32_t sub = (act && e == (uint32_t)T - 1) ? d.sub : POSW_NONE;
    Wi.act = sub != POSW_NONE;
    const Fr s = Wi.ld(sub);
    if (sub != POSW_NONE) x = fr_sub(x, s);
    return fr_sel(act, x, fr_zero());
}

// full round: T x Sigma [out | in | in2, in4], Ark [out[T] | in[T]], Mix [out[T] | in[T]].  off = FR rank of the round's first wire; cr = index of its Ark constants;
// mat = matrix.  x: element j of the lane, xb: element 4 (T = 5, lane 1).  Three batches of slots:
//   behind the squares     Sigma.in, in2, in4 of element j; T = 5: element 4's three on lanes 0, 2, 3          (3 | 4 slots)   resolved behind the S-box's last product
//                          (T = 5: at once -- held across the two x^5 products these four set the kernel's register count, 182 for 3 wavefronts per SIMD's 168)
//   behind the S-boxes     Sigma.out, Ark.in, Ark.out, Mix.in of element j                                     (4)             resolved BEFORE Mix: held across Mix's
//                          products these four load-backs cost 40 registers, the wavefront its third place on the SIMD; one exposed wait in each of 7 rounds
//   behind Mix             Mix.out of element j; T = 5: Sigma.out / Ark.in / Mix.in of element 4 on lanes 0, 2, 3 beside lane 1's Mix.out[4], and Ark.out[4] -- the
//                          two words the block goes on with stay on lane 1                                      (1 | 3)         resolved behind the next round's squares
// T = 5: 11 slots for 40 words (16 before): five quad moves and one value held across Mix against five slots of one lane in four.  A tenth slot less (Ark.out[4]
// beside the moved Sigma words) would hold a second value across Mix, where the registers peak.
template <int T, class PW> __device__ __forceinline__ void posw_full(const PW& W, uint32_t lane, uint32_t j, Fr& x, Fr& xb, uint32_t off, uint32_t cr, uint32_t mat) {
    const bool act = W.act, actb = W.actb, l1 = j == 1;
    const uint32_t jc = act ? j : 0, g0 = lane & ~3u, sg = off + 4 * j;
    const Fr x2 = fr_sqr_inl(x), x4 = fr_sqr_inl(x2);
    Fr b4 = fr_zero();
    W.template resolve<POSW_RING>();                                            // the batch before this round
    W.template put<0>(act, sg + 1, x); W.template put<1>(act, sg + 2, x2); W.template put<2>(act, sg + 3, x4);
    if constexpr (T == 5) {
        const Fr b2 = fr_sqr_inl(xb);
        b4 = fr_sqr_inl(b2);
        // lane:  0 Sigma.in[4] | 1 - | 2 Sigma.in2[4] | 3 Sigma.in4[4]
        W.template put<3>(!l1, posw_pick(j, off + 17, 0u, off + 18, off + 19), fr_sel(j == 0, posw_quad<1>(xb, g0), fr_sel(j == 2, posw_quad<1>(b2, g0), posw_quad<1>(b4, g0))));
        W.template back<4>();
    } else W.template back<3>();
    if constexpr (T == 5) W.template resolve<4>();                              // (held across x5 and element 4's x5, these four are the kernel's register peak)
    const Fr x5 = fr_mul_inl(x4, x);
    Fr y = fr_add(x5, W.kc(cr + jc));
    Fr yb = fr_zero(), h2 = fr_zero();
    if constexpr (T == 5) {
        const Fr b5 = fr_mul_inl(b4, xb);
        yb = W.vf(actb, off + 4 * T + 4, fr_add(b5, W.kc(cr + (actb ? 4u : 0u))));        // Ark.out[4]: what Mix reads; stored behind Mix
        h2 = fr_sel(j == 3, posw_quad<1>(yb, g0), posw_quad<1>(b5, g0));
    }
    if constexpr (T != 5) W.template resolve<3>();
    W.template put<0>(act, sg, x5); W.template put<1>(act, off + 5 * T + j, x5);
    y = W.template put<2>(act, off + 4 * T + j, y);                             // Ark.out: what Mix reads
    W.template put<3>(act, off + 7 * T + j, y);
    W.template back<4>();
    W.template resolve<4>();
    // Mix: element e = sum_i M[e][i] y_i, y_i broadcast inside the 4-lane group (the same y_i for both elements of a lane)
    Fr acc = fr_zero(), accb = fr_zero();
#pragma unroll 1
    for (uint32_t i = 0; i < (uint32_t)(T < 4 ? T : 4); i++) {
        const Fr yi = posw_from(y, g0 | i);
        acc = fr_add(acc, fr_mul_inl(W.kc(mat + jc * T + i), yi));
        if constexpr (T == 5) accb = fr_add(accb, fr_mul_inl(W.kc(mat + 4 * T + i), yi));
    }
    if constexpr (T == 5) {
        const Fr yi = posw_from(yb, g0 | 1u);
        acc = fr_add(acc, fr_mul_inl(W.kc(mat + jc * T + 4), yi));
        accb = fr_add(accb, fr_mul_inl(W.kc(mat + 4 * T + 4), yi));
    }
    x = W.template put<0>(act, off + 6 * T + j, acc);                           // Mix.out: the next round's input
    if constexpr (T == 5) {
        // lane:  0 Sigma.out[4] | 1 Mix.out[4] | 2 Ark.in[4] | 3 Mix.in[4]     (xb means something on lane 1 only)
        xb = W.template put<1>(true, posw_pick(j, off + 16, off + 6 * T + 4, off + 5 * T + 4, off + 7 * T + 4), fr_sel(l1, accb, h2));
        W.template put<2>(actb, off + 4 * T + 4, yb, true);                     // Ark.out[4] (its value fault taken above)
        W.template back<3>(); W.template idle<3>();
    } else { W.template back<1>(); W.template idle<1>(); }
}

template <int T, class PW> __device__ __forceinline__ void posw_run(const GArgs& A, const PosWDesc& d, const PW& W, uint32_t lane) {
    const PosOff k = pos_off(T);
    const uint32_t j = lane & 3u, base = d.base, g0 = lane & ~3u;
    const bool act = W.act, actb = W.actb, l0 = j == 0, l1 = j == 1;
    const uint32_t jc = act ? j : 0;                             // (idle slots index the table like slot 0)
    // ---- head: out | inputs[T-1] | PoseidonEx.out | PoseidonEx.inputs[T-1], initialState | Ark0 [out[T] | in[T]]: 4 slots, T = 5: a fifth for element 4
    Fr x = posw_input<T>(A, d, W, j, act), xb = fr_zero();
    W.template put<0>(act, l0 ? base + 2 * T : base + j, x);     // inputs[j-1] | lane 0: initialState = 0
    W.template put<1>(act && !l0, base + T + j, x);              // PoseidonEx.inputs[j-1]
    W.template put<2>(act, base + 3 * T + 1 + j, x);             // Ark0.in
    x = fr_add(x, W.kc(k.C + jc));
    x = W.template put<3>(act, base + 2 * T + 1 + j, x);         // Ark0.out
    W.template back<4>();
    if constexpr (T == 5) {
        const Fr i4 = posw_input<T>(A, d, W, 4, actb);
        xb = W.vf(actb, base + 2 * T + 5, fr_add(i4, W.kc(k.C + 4)));
        const Fr q4 = posw_quad<1>(i4, g0);
        W.template resolve<4>();
        // lane:  0 inputs[3] | 1 Ark0.out[4] | 2 PoseidonEx.inputs[3] | 3 Ark0.in[4]      (one value but for lane 1's)
        W.template put<0>(true, posw_pick(j, base + 4, base + 2 * T + 5, base + T + 4, base + 3 * T + 5), fr_sel(l1, xb, q4), l1);
        W.template back<1>(); W.template idle<1>();
    }
    uint32_t off = base + 4 * T + 1;
    // ---- 4 full rounds (the fourth mixes with P)
#pragma unroll 1
    for (uint32_t r = 0; r < 4; r++) { posw_full<T>(W, lane, j, x, xb, off, k.C + (r + 1) * T, r == 3 ? k.Pm : k.M); off += 8 * T; }
    // ---- partial rounds: Sigma [out | in | in2, in4] on element 0, MixS [out[T] | in[T]]; four products deep:
    //   lane 0          x^2        | x^4                    | x^5          | S_0 * s0
    //   lanes 1..T-1    S_j * x_j  | (T = 5, lane 1) the    | (T = 5,      | in_0 * S'_j
    //                              | previous round's       |  lane 1)     |
    //                              | in_0 * S'_4 into x_4   | S_4 * x_4    |
    // then out_0 = the sum over the 4 lanes (two steps).  T = 5: x_4's own in_0 * S'_4 is the one product that does not fit, so it is
    // deferred into the next round's second slot (idle on lanes 1.. otherwise); x_4's MixS.out is stored there.
    // The round's words leave in NP slots behind the S-box (the last one, MixS.out, at the round's end), their load-backs behind all of them, and the next round's S-box
    // runs before they are compared:
    //   lane                    0             1                               2            3
    //   T = 5   slot 0          Sigma.in      the previous MixS.out[4]        Sigma.in2    Sigma.in4
    //           slot 1          Sigma.out     MixS.in[4]                      -            -
    //   T < 5   slot 0          Sigma.in      Sigma.in2                       Sigma.in4    Sigma.out       (T = 3: lane 3 holds no element and carries one all the same)
    //   then    MixS.in[j], MixS.out[j] on lane j
    constexpr int NP = T == 5 ? 4 : 3;
    Fr pin0 = fr_zero();                                         // (T = 5) in_0 of the previous round
    uint32_t poff = 0;                                           // (T = 5) its first wire
#pragma unroll 1
    for (uint32_t r = 0; r < (uint32_t)k.rp; r++) {
        const uint32_t sb = k.S + (2 * T - 1) * r;
        const Fr c1 = W.kc(sb + jc);
        const Fr m1 = fr_mul_inl(x, fr_sel(l0, x, c1));                    // x^2 | S_j * x_j
        W.template resolve<NP>();                                    // the batch before this round, behind this round's first product: held across all three of the
                                                                     // S-box the load-backs cost the wavefront its third place on the SIMD (the last full round left slots 1.. or 3 idle)
        Fr m2, m3;
        if constexpr (T == 5) {
            const Fr cp = W.kc(r ? sb - (2 * T - 1) + T + 3 : sb);
            m2 = fr_mul_inl(fr_sel(l0, m1, pin0), fr_sel(l0, m1, cp));           // x^4 | in_0' * S'_4'
            if (r) xb = W.vf(actb, poff + 4 + 4, fr_add(xb, m2));                // the previous round's MixS.out[4]: stored in slot 0
            m3 = fr_mul_inl(fr_sel(l0, m2, xb), fr_sel(l0, x, W.kc(sb + 4)));    // x^5 | S_4 * x_4
        } else {
            m2 = fr_sqr_inl(m1);                                     // x^4 (lane 0 only)
            m3 = fr_mul_inl(m2, x);                                  // x^5 (lane 0 only)
        }
        const Fr s0 = fr_add(m3, W.kc(k.C + 5 * T + r));
        const Fr q1 = posw_quad<0>(m1, g0), q2 = posw_quad<0>(m2, g0);
        if constexpr (T == 5) {
            W.template put<0>(!l1 || r != 0, posw_pick(j, off + 1, poff + 4 + 4, off + 2, off + 3), posw_pick(j, x, xb, q1, q2), l1);
            W.template put<1>(j < 2, l0 ? off : off + 4 + T + 4, fr_sel(l0, m3, xb));
        } else {
            W.template put<0>(true, posw_pick(j, off + 1, off + 2, off + 3, off), posw_pick(j, x, q1, q2, posw_quad<0>(m3, g0)));
        }
        W.template put<NP - 2>(act, off + 4 + T + j, fr_sel(l0, s0, x));        // MixS.in
        const Fr in0 = posw_from(s0, g0);
        const Fr c2 = W.kc(jc == 0 ? sb : sb + T + jc - 1);
        const Fr m4 = fr_mul_inl(c2, in0);                           // S_0 * s0 | in_0 * S'_j
        Fr part = fr_sel(l0, m4, m1);
        if constexpr (T == 5) if (actb) part = fr_add(part, m3);
        if (!act) part = fr_zero();
        const Fr sum = posw_group_sum(part, lane);
        x = fr_sel(l0, sum, fr_add(x, m4));
        x = W.template put<NP - 1>(act, off + 4 + j, x);             // MixS.out
        W.template back<NP>();
        if constexpr (T == 5) { pin0 = in0; poff = off; }
        off += 4 + 2 * T;
    }
    if constexpr (T == 5) {                                      // the last round's deferred in_0 * S'_4
        xb = fr_add(xb, fr_mul_inl(pin0, W.kc(k.S + (2 * T - 1) * (k.rp - 1) + T + 3)));
        W.template resolve<NP>();
        xb = W.template put<0>(actb, poff + 4 + 4, xb);
        W.template back<1>(); W.template idle<1>();
    } else W.template idle<NP>();
    // ---- 3 full rounds
#pragma unroll 1
    for (uint32_t r = 0; r < 3; r++) { posw_full<T>(W, lane, j, x, xb, off, k.C + 5 * T + k.rp + r * T, k.M); off += 8 * T; }
    // ---- tail: T x Sigma, MixLast [out | in[T]], PoseidonEx.out, out (and the caller's copy of the hash)
    // Three batches: Sigma.in / in2 / in4 (T = 5: + element 4's four Sigma words on the four lanes), Sigma.out and MixLast.in (T = 5: + MixLast.in[4]), and ONE slot
    // for the hash's four copies -- the group's sum stands in every lane
    {
        const Fr x2 = fr_sqr_inl(x), x4 = fr_sqr_inl(x2);
        const uint32_t sg = off + 4 * j;
        Fr b5 = fr_zero();
        W.template resolve<POSW_RING>();
        W.template put<0>(act, sg + 1, x); W.template put<1>(act, sg + 2, x2); W.template put<2>(act, sg + 3, x4);
        if constexpr (T == 5) {
            const Fr b2 = fr_sqr_inl(xb), b4 = fr_sqr_inl(b2);
            b5 = fr_mul_inl(b4, xb);
            // lane:  0 Sigma.in2[4] | 1 Sigma.in[4] | 2 Sigma.in4[4] | 3 Sigma.out[4]
            W.template put<3>(true, posw_pick(j, off + 18, off + 17, off + 19, off + 16), posw_pick(j, posw_quad<1>(b2, g0), xb, posw_quad<1>(b4, g0), posw_quad<1>(b5, g0)));
            W.template back<4>();
        } else W.template back<3>();
        const Fr x5 = fr_mul_inl(x4, x);
        Fr part = fr_mul_inl(W.kc(k.M + jc), x5);
        if constexpr (T == 5) {
            const Fr pb = fr_mul_inl(W.kc(k.M + 4), b5);
            if (actb) part = fr_add(part, pb);
        }
        if (!act) part = fr_zero();
        W.template resolve<T == 5 ? 4 : 3>();
        W.template put<0>(act, sg, x5);
        W.template put<1>(act, off + 4 * T + 1 + j, x5);             // MixLast.in
        if constexpr (T == 5) { W.template put<2>(actb, off + 4 * T + 5, b5); W.template back<3>(); } else W.template back<2>();
        const Fr h = posw_group_sum(part, lane);
        W.template resolve<T == 5 ? 3 : 2>();
        // lane:  0 MixLast.out | 1 PoseidonEx.out | 2 out | 3 the caller's copy
        W.template put<0>(j < 3 || d.also != POSW_NONE, posw_pick(j, off + 4 * T, base + T, base, d.also), h);
        W.template back<1>();
        W.template resolve<1, 0>(j == 3);
    }
}

// (which elements a value fault may be armed on -- where posw_run goes on with what put() / vf() return: circuits.hpp posw_value_fault_covers)
// bx = 4 * unit + witness slice (unit = position in the launch's list), g = group; the wavefronts of a workgroup have the same unit
#define POSW_SLICES 4              // wavefronts per (unit, group): 16 witnesses each
#ifndef POSW_WAVES
#define POSW_WAVES 4
#endif
static_assert(POSW_SLICES % POSW_WAVES == 0, "the slices of a workgroup belong to one unit");
template <bool RIDE, bool FAULT = false> __device__ __forceinline__ void poswide_body(const GArgs& A, uint32_t bx, uint32_t g) {
#ifdef POSW_KNOCKOUT               // measurement builds only (tools/build_variant.py g_gen_poswide.hip:-DPOSW_KNOCKOUT): the Poseidon wavefronts return at once -- the bound
    return;                        // on what the step can gain from them (profiles/pos_slots_ab.txt); the records of such a build are wrong
#endif
    __builtin_amdgcn_s_setprio(3);
    const uint32_t lane = threadIdx.x & 63u;
    const UnitDesc* dp = A.units + POB_UNI(A.order[A.first + bx / POSW_SLICES]);
    const int T = (int)POB_UNI(dp->a[0]);
    const PosWDesc d = {POB_UNI(dp->cur.f), POB_UNI(dp->a[1]), POB_UNI(dp->a[2]), POB_UNI(dp->a[3]), POB_UNI(dp->a[4]), POB_UNI(dp->a[5]), POB_UNI(dp->a[6])};
    const PosOff k = pos_off(T);
    const uint32_t kend = T == 3 ? POS_OFF_C_4 : T == 4 ? POS_OFF_C_5 : POS_TABLE_LEN;     // the constants of one T are contiguous
    for (uint32_t i = threadIdx.x; i < (kend - k.C) * 8; i += blockDim.x) g_lds[i] = A.pos_tab[(size_t)k.C * 8 + i];
    __syncthreads();
    PosWideT<RIDE, FAULT> W;
    uint32_t* frp = A.fr + (uint64_t)g * A.fr_stride;
    const uint64_t nf = A.fr_stride * 4;
    W.rs = __builtin_amdgcn_make_buffer_rsrc(frp, 0, (int)(nf > 0xFFFFF000ull ? 0xFFFFF000ull : nf), 0x00020000);
    const uint32_t slot = 16 * (bx % POSW_SLICES) + (lane >> 2);           // the lane's witness in the group
    W.slot4 = slot * 4;
    W.act = (lane & 3u) < (uint32_t)T;
    W.actb = T == 5 && (lane & 3u) == 1;
    W.ktab = g_lds; W.kbase = k.C;
    W.w_of_f = POB_UNI(dp->cur.w) - d.base; W.w_also = POB_UNI(dp->cur.w);
    if constexpr (RIDE) W.ride_init();
    if constexpr (FAULT) { W.fault_f = A.fault_idx; W.fault_me = (A.fault_cls & 0xFFu) == 2 && g == A.fault_group && ((A.fault_lanes >> slot) & 1); W.fault_val = (A.fault_cls & FAULT_VALUE) != 0; }
    if (T == 3) posw_run<3>(A, d, W, lane); else if (T == 4) posw_run<4>(A, d, W, lane); else posw_run<5>(A, d, W, lane);
    if constexpr (RIDE) {          // (posw_run resolved its last slot) the lowest differing wire over the 4 lanes of a witness, reported by its first lane
        uint32_t b = W.bad;
#pragma unroll
        for (uint32_t m = 2; m >= 1; m >>= 1) { const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ m) << 2), (int)b); b = o < b ? o : b; }
        if ((lane & 3u) == 0 && b != 0xFFFFFFFFu) atomicMin(&A.bad_wire[g * 64 + slot], b);
    }
}
// grid = (POSW_SLICES / POSW_WAVES * nunits, ngroups) workgroups of POSW_WAVES wavefronts
template <bool RIDE, bool FAULT> __global__ void __launch_bounds__(64 * POSW_WAVES) k_poseidon_wide(GArgs A) { poswide_body<RIDE, FAULT>(A, POSW_WAVES * blockIdx.x + (threadIdx.x >> 6), blockIdx.y); }
static_assert(POS_TABLE_LEN - POS_OFF_C_5 >= POS_OFF_C_5 - POS_OFF_C_4 && POS_TABLE_LEN - POS_OFF_C_5 >= POS_OFF_C_4 - POS_OFF_C_3, "the T = 5 constants are the largest set");
#define POSW_LDS_BYTES ((POS_TABLE_LEN - POS_OFF_C_5) * 32u)
