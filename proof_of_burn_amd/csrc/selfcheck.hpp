// Emit-time self-check: where a wire lies in an emission window and ONE statement of every relation of the derived wires, shared by the single-witness kernels
// (pob_host.hip k_selfcheck_*) and the group kernels (k_selfcheck_group.hip), which evaluate them on witness l's window of the group's canonical scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_common.hpp"

// where wire w lies in the window: O0 (rbits null) position w - w0; reduced witness: its rank among the kept wires - w0, false if the wire is dropped
struct ScWin { const uint8_t* win; uint32_t w0, wn; const unsigned long long* rbits; const uint32_t* rpre; };
// the group's 64 windows (witness l's at win + l * plane; bit l of lanes = witness l is emitted) and where the verdicts go: bad[64] = per lane of the group the lowest
// violated wire (0xFFFFFFFF = none), cnt = {sites skipped, sites evaluated} per witness
struct ScGroup { const uint8_t* win; uint64_t plane, lanes; uint32_t w0, wn; const unsigned long long* rbits; const uint32_t* rpre; uint32_t* bad; uint32_t* cnt; };
// grid = (ceil(n / 64), popcount(lanes)), behind the last writer of the scratch on st.  O0 form: z = IsZero words (bit 31: child of an IsEqual), m = M triples, c = copy pairs;
// reduced form: zr = lists of six wires, mr = of four (pob_host.hip builds both per map)
void launch_selfcheck_group_z(const ScGroup& G, const uint32_t* sites, uint32_t n, hipStream_t st);
void launch_selfcheck_group_c(const ScGroup& G, const uint32_t* sites, uint32_t n, hipStream_t st);
void launch_selfcheck_group_m(const ScGroup& G, const uint32_t* sites, uint32_t n, const uint32_t* pow256, hipStream_t st);
void launch_selfcheck_group_zr(const ScGroup& G, const uint32_t* zw, uint32_t n, hipStream_t st);
void launch_selfcheck_group_mr(const ScGroup& G, const uint32_t* mw, uint32_t n, const uint32_t* pow256, hipStream_t st);
// test hook (pob_debug_group_emit_xor): one byte of the scratch XORed with mask by a one-thread kernel
void launch_group_xor_byte(uint8_t* p, uint8_t mask, hipStream_t st);

#ifdef __HIPCC__
__device__ __forceinline__ bool sc_pos(const ScWin& W, uint32_t w, uint32_t* pos) {
    if (!W.rbits) { *pos = w - W.w0; return *pos < W.wn; }
    const unsigned long long word = W.rbits[w >> 6];
    if (!((word >> (w & 63)) & 1)) return false;
    *pos = W.rpre[w >> 6] + (uint32_t)__popcll(word & ((1ull << (w & 63)) - 1)) - W.w0;
    return *pos < W.wn;
}
__device__ __forceinline__ Fr sc_load(const ScWin& W, uint32_t pos) {
    const uint32_t* q = (const uint32_t*)(W.win + (size_t)pos * 32);
    Fr c; for (int j = 0; j < 8; j++) c.l[j] = q[j];
    return fr_to_mont(c);
}

// What became of a site in this window.  SC_NONE: not this window's (reduced lists: the first wire lies elsewhere); SC_SKIP: a wire outside the window or dropped;
// SC_OK / SC_BAD: evaluated, *wire = the wire that names the site
enum { SC_NONE = 0, SC_SKIP = 1, SC_OK = 2, SC_BAD = 3 };
// IsZero [out | in | inv] at w (s = w | bit 31: child of an IsEqual [out | in[2]] at w - 3)
__device__ __forceinline__ uint32_t sc_rel_z(const ScWin& W, uint32_t s, uint32_t* wire) {
    const uint32_t w = s & 0x7FFFFFFFu;
    uint32_t po, pi, pv, pe = 0, pa = 0, pb = 0;
    bool have = sc_pos(W, w, &po) && sc_pos(W, w + 1, &pi) && sc_pos(W, w + 2, &pv);
    if (have && (s >> 31)) have = sc_pos(W, w - 3, &pe) && sc_pos(W, w - 2, &pa) && sc_pos(W, w - 1, &pb);
    if (!have) return SC_SKIP;
    *wire = w;
    const Fr out = sc_load(W, po), in = sc_load(W, pi), inv = sc_load(W, pv);
    bool ok = fr_eq(fr_mul(in, inv), fr_sub(fr_one_mont(), out)) && fr_is_zero(fr_mul(in, out));
    if (s >> 31) {
        const Fr eo = sc_load(W, pe), a = sc_load(W, pa), b = sc_load(W, pb);
        ok = ok && fr_eq(in, fr_sub(b, a)) && fr_eq(eo, out);
    }
    return ok ? SC_OK : SC_BAD;
}
// copy constraint a === b between a derived wire and the stored wire it must equal (a: the higher wire)
__device__ __forceinline__ uint32_t sc_rel_c(const ScWin& W, uint32_t a, uint32_t b, uint32_t* wire) {
    uint32_t pa, pb;
    if (!sc_pos(W, a, &pa) || !sc_pos(W, b, &pb)) return SC_SKIP;      // (the lower wire lies in the window before, or one of the two is dropped)
    *wire = a;
    const uint4* p = (const uint4*)(W.win + (size_t)pa * 32); const uint4* q = (const uint4*)(W.win + (size_t)pb * 32);
    const uint4 x0 = p[0], x1 = p[1], y0 = q[0], y1 = q[1];
    return (x0.x != y0.x || x0.y != y0.y || x0.z != y0.z || x0.w != y0.w || x1.x != y1.x || x1.y != y1.y || x1.z != y1.z || x1.w != y1.w) ? SC_BAD : SC_OK;
}
// M[k+1] (wire wn1) === M[k] (wn1 - 1) + mainInput[k] (wb) * 256^k
__device__ __forceinline__ uint32_t sc_rel_m(const ScWin& W, uint32_t wn1, uint32_t wb, uint32_t k, const uint32_t* pow256, uint32_t* wire) {
    uint32_t pn, pp, pby;
    if (!sc_pos(W, wn1, &pn) || !sc_pos(W, wn1 - 1, &pp) || !sc_pos(W, wb, &pby)) return SC_SKIP;
    *wire = wn1;
    Fr pw; for (int j = 0; j < 8; j++) pw.l[j] = pow256[(size_t)k * 8 + j];                      // 256^k, Montgomery
    const Fr next = sc_load(W, pn), prev = sc_load(W, pp), by = sc_load(W, pby);
    return fr_eq(next, fr_add(prev, fr_mul(by, pw))) ? SC_OK : SC_BAD;
}
// the same relations on explicit wire lists (reduced witness): every wire of a site is kept (the host left the others out); a site is evaluated in the window that holds
// its first wire -- if the others lie there too.  w6: IsZero out, in, inv | IsEqual out, in[0], in[1] (0xFFFFFFFF: a bare IsZero); an entry with bit 31 set: a wire pinned
// to the small constant in its low bits -- not in the window at all
__device__ __forceinline__ uint32_t sc_rel_zr(const ScWin& W, const uint32_t* w6, uint32_t* wire) {
    uint32_t p[6];
    if (!sc_pos(W, w6[0], &p[0])) return SC_NONE;
    const bool iseq = w6[3] != 0xFFFFFFFFu;
    auto pos = [&](int j) { if (w6[j] >> 31) { p[j] = w6[j]; return true; } return sc_pos(W, w6[j], &p[j]); };
    bool have = pos(1) && pos(2);
    if (have && iseq) have = pos(3) && pos(4) && pos(5);
    if (!have) return SC_SKIP;
    *wire = w6[0];
    auto val = [&](int j) { if (p[j] >> 31) { Fr c = fr_zero(); c.l[0] = p[j] & 0x7FFFFFFFu; return fr_to_mont(c); } return sc_load(W, p[j]); };
    const Fr out = val(0), in = val(1), inv = val(2);
    bool ok = fr_eq(fr_mul(in, inv), fr_sub(fr_one_mont(), out)) && fr_is_zero(fr_mul(in, out));
    if (iseq) { const Fr eo = val(3), a = val(4), b = val(5); ok = ok && fr_eq(in, fr_sub(b, a)) && fr_eq(eo, out); }
    return ok ? SC_OK : SC_BAD;
}
// w4: M[k+1], M[k], mainInput[k], k
__device__ __forceinline__ uint32_t sc_rel_mr(const ScWin& W, const uint32_t* w4, const uint32_t* pow256, uint32_t* wire) {
    uint32_t pn, pp, pby;
    if (!sc_pos(W, w4[0], &pn)) return SC_NONE;
    if (!sc_pos(W, w4[1], &pp) || !sc_pos(W, w4[2], &pby)) return SC_SKIP;
    *wire = w4[0];
    Fr pw; for (int j = 0; j < 8; j++) pw.l[j] = pow256[(size_t)w4[3] * 8 + j];
    const Fr next = sc_load(W, pn), prev = sc_load(W, pp), by = sc_load(W, pby);
    return fr_eq(next, fr_add(prev, fr_mul(by, pw))) ? SC_OK : SC_BAD;
}
#endif  // __HIPCC__
