// libpob_hip.so -- the .wtns emission: window pipeline of the single-witness paths (canonical, reduced, packed), group emission, both self-checks, the .wtns writers
// and the emission's measurements and test hooks.  The handle and the helpers shared with pob_host.hip: pob_ctx.hpp.
#include "pob_ctx.hpp"

// the window-sized buffers of the group emission: freed and forgotten (no early return: every pointer is null afterwards, whatever a free reports)
static void group_free_device(EmitGroup& Gr) {
    for (void* p : {(void*)Gr.d_win, (void*)Gr.d_pk[0], (void*)Gr.d_pk[1], (void*)Gr.d_hdr[0], (void*)Gr.d_hdr[1], (void*)Gr.d_blk, (void*)Gr.d_tot}) if (p) (void)hipFree(p);
    for (uint8_t* p : {Gr.h_hdr[0], Gr.h_hdr[1]}) if (p) (void)hipHostFree(p);
    Gr.d_win = Gr.d_pk[0] = Gr.d_pk[1] = Gr.d_hdr[0] = Gr.d_hdr[1] = Gr.h_hdr[0] = Gr.h_hdr[1] = nullptr; Gr.d_blk = Gr.d_tot = nullptr; Gr.alloc_wires = 0;
}
// pob_close: everything the emission allocated or created, but for its two streams (freed while the device may still be busy, as the handle's other buffers are) ...
void pob_detail::emit_release(pob_ctx* h) {
    EmitState& E = h->em;
    void* ptrs[] = {E.d_win[0], E.d_win[1], E.d_win[2], E.d_order, E.d_probe, E.d_rbits, E.d_rpre, E.d_sc_res, E.d_sc_zr, E.d_sc_mr, E.d_gsc_res, E.d_pk[0], E.d_pk[1], E.d_pk[2], E.d_pk_blk, E.d_pk_tot};
    for (void* p : ptrs) if (p) hipFree(p);
    E.sc.free(); E.gsc.free();
    {
        EmitGroup& Gr = E.grp;
        group_free_device(Gr);
        for (int k = 0; k < 3; k++) if (Gr.h_pin[k]) hipHostFree(Gr.h_pin[k]);
        for (hipEvent_t e : {Gr.ev_made[0], Gr.ev_made[1], Gr.ev_hdr[0], Gr.ev_hdr[1], Gr.ev_free[0], Gr.ev_free[1], Gr.ev_copied[0], Gr.ev_copied[1], Gr.ev_copied[2]}) if (e) hipEventDestroy(e);
    }
    for (int k = 0; k < EmitState::NSLOT; k++) {
        if (E.h_pin[k]) hipHostFree(E.h_pin[k]);
        for (hipEvent_t e : {E.ev_made[k], E.ev_copied[k], E.ev_free[k]}) if (e) hipEventDestroy(e);
    }
}
// ... and the streams, once the device is idle
void pob_detail::emit_release_streams(pob_ctx* h) {
    if (h->em.s_copy) hipStreamDestroy(h->em.s_copy);
    if (h->em.s_val) hipStreamDestroy(h->em.s_val);
}

// ---- what the single-witness and the group paths share
// The emitting G units through `launch` (launch_g_emit | launch_g_emit_group), A.first / A.order set per launch: for window k only the units that the probe pass found
// writing into it -- if its tables are for the window size and map in effect and have that window --, else every unit (k = EMIT_ALL_UNITS: the probe and recording passes)
#define EMIT_ALL_UNITS (~0ull)
static void emit_units(pob_ctx* h, GArgs A, uint64_t k, void (*launch)(const GArgs&, uint32_t, uint32_t, hipStream_t)) {
    const EmitState& E = h->em;
    hipStream_t st = own_stream(h);
    if (E.probe_win == E.win_wires && E.probe_map == E.map_id && k < E.wsegs.size()) {
        A.order = E.d_order;
        for (const EmitState::WSeg& sg : E.wsegs[k]) { A.first = sg.first; launch(A, sg.cls, sg.count, st); }
    } else {
        for (const pob_ctx::Seg& sg : h->emit_segs) { A.first = sg.first; launch(A, sg.lds, sg.count, st); }
    }
}
// The Keccak kernels' wires of the window of positions [w0, w0 + wn): f(run, lo, hi) for every run with wires there, [lo, hi) = the run cut to the window's wire range --
// reduced form: from its first to its last kept wire of the window; a run without one is skipped (a round block whose wires are all dropped costs nothing)
template <class F> static void for_each_run_piece(const EmitState& E, uint64_t w0, uint64_t wn, F f) {
    const uint64_t wire_lo = E.red ? E.keep[w0] : w0, wire_hi = E.red ? (uint64_t)E.keep[w0 + wn - 1] + 1 : w0 + wn;
    for (const EmitState::Run& r : E.runs) {
        uint64_t lo = std::max<uint64_t>(r.w, wire_lo), hi = std::min<uint64_t>((uint64_t)r.w + r.n, wire_hi);
        if (lo >= hi) continue;
        if (E.red) {
            const auto a = std::lower_bound(E.keep.begin() + w0, E.keep.begin() + w0 + wn, (uint32_t)lo), b = std::lower_bound(a, E.keep.begin() + w0 + wn, (uint32_t)hi);
            if (a == b) continue;
            lo = *a; hi = (uint64_t)*(b - 1) + 1;
        }
        f(r, lo, hi);
    }
}
hipError_t SiteTables::upload(const std::vector<std::array<uint32_t, 3>>& ms, const std::vector<std::array<uint32_t, 2>>& cs) {
    m_next.resize(ms.size()); c_hi.resize(cs.size());
    for (size_t i = 0; i < ms.size(); i++) m_next[i] = ms[i][0];
    for (size_t i = 0; i < cs.size(); i++) c_hi[i] = cs[i][0];
    hipError_t e = hipMalloc(&d_z, std::max<size_t>(z.size(), 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&d_m, std::max<size_t>(ms.size(), 1) * 12);
    if (e == hipSuccess) e = hipMalloc(&d_c, std::max<size_t>(cs.size(), 1) * 8);
    if (e == hipSuccess && !z.empty()) e = hipMemcpy(d_z, z.data(), z.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !ms.empty()) e = hipMemcpy(d_m, ms.data(), ms.size() * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess && !cs.empty()) e = hipMemcpy(d_c, cs.data(), cs.size() * 8, hipMemcpyHostToDevice);
    return e;
}
void SiteTables::free() {
    for (uint32_t** q : {&d_z, &d_m, &d_c}) { if (*q) (void)hipFree(*q); *q = nullptr; }
}
SiteTables::Window SiteTables::window(uint64_t wire_lo, uint64_t wire_hi) const {
    const auto zless = [](uint32_t s, uint32_t v) { return (s & 0x7FFFFFFFu) < v; };
    const auto za = std::lower_bound(z.begin(), z.end(), (uint32_t)wire_lo, zless), zb = std::lower_bound(za, z.end(), (uint32_t)wire_hi, zless);
    const auto ma = std::lower_bound(m_next.begin(), m_next.end(), (uint32_t)wire_lo), mb = std::lower_bound(ma, m_next.end(), (uint32_t)wire_hi);      // M sites whose M[k+1] lies in the range
    const auto ca = std::lower_bound(c_hi.begin(), c_hi.end(), (uint32_t)wire_lo), cb = std::lower_bound(ca, c_hi.end(), (uint32_t)wire_hi);              // copy sites whose HIGHER wire does
    return {{d_z + (za - z.begin()), (uint32_t)(zb - za)}, {d_m + 3 * (ma - m_next.begin()), (uint32_t)(mb - ma)}, {d_c + 2 * (ca - c_hi.begin()), (uint32_t)(cb - ca)}};
}

extern "C" {

// ---- streaming emission (reference: writeBinWitness, patch point tests/test.py:36).  The canonical payload (32 B per wire: 6.9 GB for
// the production instantiation) never exists on the device as a whole: it is expanded window by window from the compact resident
// vector, each window goes D2H into pinned memory on a copy stream while the next one is being expanded and the caller consumes
// the previous one.
static int emit_make_window(pob_ctx* h, uint32_t idx, uint64_t k, int slot) {
    EmitState& E = h->em;
    const uint64_t w0 = k * E.win_wires, wn = std::min(E.win_wires, E.total - w0);      // positions of the payload (kept wires in reduced mode)
    hipStream_t st = own_stream(h);
    HIPC(hipStreamWaitEvent(st, E.ev_free[slot], 0));                       // the copy of the window that used this slot before is done
    // any wire nobody owns stays 0xEE.. (not a field element: the byte compare with the oracle catches it); rocclr's fill kernel took
    // 4.5 ms per 256 MiB window, this one runs at the HBM write rate
    hipLaunchKernelGGL(k_fill_ee, dim3(2048), dim3(256), 0, st, (uint4*)E.d_win[slot], wn * 2);
    if (w0 == 0) { const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0}; HIPC(hipMemcpyAsync(E.d_win[slot], one, 32, hipMemcpyHostToDevice, st)); }   // wire 0 = 1 (always kept)
    GArgs A = gargs(h);
    A.emit_out = E.d_win[slot]; A.emit_sel = idx % 64; A.emit_group = idx / 64; A.emit_w0 = (uint32_t)w0; A.emit_wn = (uint32_t)wn;
    if (E.red) { A.emit_rbits = E.d_rbits; A.emit_rpre = E.d_rpre; }
    emit_units(h, A, k, launch_g_emit);
    const u64* Gp = (const u64*)h->d_bits + (uint64_t)(idx / 64) * h->plan.bit_stride;
    for_each_run_piece(E, w0, wn, [&](const EmitState::Run& r, uint64_t lo, uint64_t hi) {       // the Keccak kernels' wires
        if (!E.red) {
            if (r.absorb) launch_k_emit_absorb(Gp, E.d_win[slot] + (lo - w0) * 32, AbsorbRef{r.b, r.prev, r.src}, r.o + (uint32_t)(lo - r.w), (uint32_t)(hi - lo), idx % 64, h->d_ktab, st);
            else launch_k_emit_bits(Gp, E.d_win[slot] + (lo - w0) * 32, 0, (uint32_t)(r.b + (lo - r.w)), (uint32_t)(hi - lo), idx % 64, st);
        } else {
            if (r.absorb) launch_k_emit_absorb_red(Gp, E.d_win[slot], (uint32_t)lo, AbsorbRef{r.b, r.prev, r.src}, r.o + (uint32_t)(lo - r.w), (uint32_t)(hi - lo), idx % 64, h->d_ktab, E.d_rbits, E.d_rpre, (uint32_t)w0, (uint32_t)wn, st);
            else launch_k_emit_bits_red(Gp, E.d_win[slot], (uint32_t)lo, (uint32_t)(r.b + (lo - r.w)), (uint32_t)(hi - lo), idx % 64, E.d_rbits, E.d_rpre, (uint32_t)w0, (uint32_t)wn, st);
        }
    });
    if (E.sc_on && E.red) {   // reduced witness: every site whose wires are all kept (through their class representatives), at their ranks (lists built in emit_start)
        const ScWin W{E.d_win[slot], (uint32_t)w0, (uint32_t)wn, E.d_rbits, E.d_rpre};
        uint32_t* res = E.d_sc_res; const uint32_t* zr = E.d_sc_zr; const uint32_t* mr = E.d_sc_mr; const uint32_t* pw = h->d_pow256; const uint32_t nz = E.sc_red_nz, nm = E.sc_red_nm;
        if (nz) hipLaunchKernelGGL(k_selfcheck_zr, dim3((nz + 63) / 64), dim3(64), 0, st, W, zr, nz, res);
        if (nm) hipLaunchKernelGGL(k_selfcheck_mr, dim3((nm + 63) / 64), dim3(64), 0, st, W, mr, nm, pw, res);
    }
    if (E.sc_on && !E.red) {        // the derived wires' relations on the values just written into this window
        const ScWin W{E.d_win[slot], (uint32_t)w0, (uint32_t)wn, nullptr, nullptr};
        uint32_t* res = E.d_sc_res;
        // sites by the wire range of the window (O0: position = wire); the kernels skip (and count) a site one of whose wires is outside the window
        const SiteTables::Window S = E.sc.window(w0, w0 + wn);
        const uint32_t nz = S.z.n, nm = S.m.n, ncs = S.c.n;             // (plain locals: the CPU shim's launch macro evaluates its arguments inside a by-copy lambda)
        const uint32_t *zs = S.z.p, *msites = S.m.p, *csites = S.c.p, *pw = h->d_pow256;
        if (nz) hipLaunchKernelGGL(k_selfcheck_z, dim3((nz + 63) / 64), dim3(64), 0, st, W, zs, nz, res);
        if (nm) hipLaunchKernelGGL(k_selfcheck_m, dim3((nm + 63) / 64), dim3(64), 0, st, W, msites, nm, pw, res);
        if (ncs) hipLaunchKernelGGL(k_selfcheck_c, dim3((ncs + 63) / 64), dim3(64), 0, st, W, csites, ncs, res);
        E.sc_checked += S.total();
    }
    HIPC(hipGetLastError());
    if (E.packed) {           // behind everything that writes (and checks) the canonical window: compact it; what crosses now is the part whose length does not depend on the values
        launch_pack_window(E.d_win[slot], w0, (uint32_t)wn, E.d_pk[slot], E.d_pk_blk, E.d_pk_tot, st);
        HIPC(hipGetLastError());
    }
    HIPC(hipEventRecord(E.ev_made[slot], st));
    HIPC(hipStreamWaitEvent(E.s_copy, E.ev_made[slot], 0));
    if (E.packed) { HIPC(hipMemcpyAsync(E.h_pin[slot], E.d_pk[slot], pack_fixed_bytes(wn), hipMemcpyDeviceToHost, E.s_copy)); E.pk_d2h += pack_fixed_bytes(wn); }
    else HIPC(hipMemcpyAsync(E.h_pin[slot], E.d_win[slot], wn * 32, hipMemcpyDeviceToHost, E.s_copy));
    HIPC(hipEventRecord(E.ev_copied[slot], E.s_copy));
    HIPC(hipEventRecord(E.ev_free[slot], E.s_copy));
    return POB_OK;
}

static uint64_t fnv64(const void* p, size_t n) {
    const uint8_t* q = (const uint8_t*)p; uint64_t hsh = 1469598103934665603ull;
    // (8 bytes at a time: the map of a production witness has ~20 M entries)
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t v; memcpy(&v, q + i, 8); hsh = (hsh ^ v) * 1099511628211ull; }
    for (; i < n; i++) hsh = (hsh ^ q[i]) * 1099511628211ull;
    return hsh ? hsh : 1;
}

// the generation statuses of the current batch on the host (one D2H per generation): no witness is emitted for a failed input
static int emit_statuses(pob_ctx* h) {
    EmitState& E = h->em;
    if (E.status_gen == h->gen_count && E.status_host.size() == h->n) return POB_OK;
    HIPC(hipEventSynchronize(h->ev_gen_done));
    E.status_host.resize(h->n);
    HIPC(hipMemcpyAsync(E.status_host.data(), h->d_status, (size_t)h->n * 4, hipMemcpyDeviceToHost, own_stream(h)));
    HIPC(hipStreamSynchronize(own_stream(h)));
    E.status_gen = h->gen_count;
    return POB_OK;
}

// common head of every begin: this handle's work only (a partner handle may be busy) -- the generation of the batch and its evaluation -- is done and the batch's statuses are
// on the host; the window size in effect for a payload of `total` positions (0: default_window; never more than the payload) and the number of windows
static int emit_prepare(pob_ctx* h, uint64_t total, uint64_t default_window, uint64_t* window_wires, uint64_t* nwin) {
    HIPC(hipEventSynchronize(h->ev_gen_done));
    if (h->evaluated) HIPC(hipEventSynchronize(h->ev_check_done));
    { int rc = emit_statuses(h); if (rc) return rc; }
    if (*window_wires == 0) *window_wires = default_window;
    *window_wires = std::min<uint64_t>(*window_wires, total);
    *nwin = (total + *window_wires - 1) / *window_wires;
    return POB_OK;
}

// the copy stream, the slots' events and the Keccak kernels' runs: once per handle; the copies of a previous emission (an abandoned one, a discarded first window) are waited for
static int emit_streams_and_runs(pob_ctx* h) {
    EmitState& E = h->em;
    const int NS = EmitState::NSLOT;
    if (E.s_copy) HIPC(hipStreamSynchronize(E.s_copy));
    if (!E.s_copy) {
        HIPC(hipStreamCreateWithPriority(&E.s_copy, hipStreamNonBlocking, 0));
        for (int k = 0; k < NS; k++) {
            HIPC(hipEventCreateWithFlags(&E.ev_made[k], hipEventDisableTiming)); HIPC(hipEventCreateWithFlags(&E.ev_copied[k], hipEventDisableTiming));
            HIPC(hipEventCreateWithFlags(&E.ev_free[k], hipEventDisableTiming));
        }
        for (const SpongeDesc& sp : h->plan.sponges) {
            // Keccak.in / Final.in: copies of KeccakBytes.inBlocks; Final.s[0] = Absorb 0's s (zero: expanded through the block's alias map), Final.s[b + 1] = block b's stored midRound[24]
            E.runs.push_back({sp.kin_w, sp.src_b, sp.n * 1088, 0, 0, 0, 0}); E.runs.push_back({sp.fin_w, sp.src_b, sp.n * 1088, 0, 0, 0, 0});
            E.runs.push_back({sp.fs_w, sp.abs_b, 1600, 1, 1600, NO_RANK, sp.src_b});
            for (uint32_t b = 0; b < sp.n; b++) {
                const uint32_t ab = sp.abs_b + b * ABSORB_BITS, m24 = ab + AB_MID + 24u * 1600u;
                E.runs.push_back({sp.fs_w + (b + 1) * 1600, m24, 1600, 0, 0, 0, 0});
                E.runs.push_back({sp.abs_w + b * ABSORB_WIRES, ab, ABSORB_WIRES, 1, 0, b ? m24 - ABSORB_BITS : NO_RANK, sp.src_b + b * 1088});
            }
        }
        std::sort(E.runs.begin(), E.runs.end(), [](const EmitState::Run& a, const EmitState::Run& b) { return a.w < b.w; });
    }
    return POB_OK;
}

// which G units write into which window: one probe pass per (window size, map), with the single-witness kernels (what a unit writes does not depend on the witness)
static int emit_probe_pass(pob_ctx* h, uint32_t group, uint64_t window_wires, uint64_t nwin_);

// the self-check's site tables (layout constants of the handle; both switches, pob_emit_selfcheck and pob_emit_group_selfcheck, use them): the recording pass is the
// single-witness emitter's (EmitPT<false>), run for witness idx (what it records does not depend on the witness)
static int sc_record_sites(pob_ctx* h, uint32_t idx) {
    EmitState& E = h->em;
    E.sc.free(); if (E.d_sc_res) { (void)hipFree(E.d_sc_res); E.d_sc_res = nullptr; }      // (what an earlier attempt that failed half-way left behind: sc_built is still false)
    // site-recording pass: every emitting unit once with EmitP::sites set (nothing is written); the sites are layout constants of the handle
    const uint32_t cap = std::max(h->plan.total.q, 1u);
    uint32_t* d_rec = nullptr;
    const size_t words = 4 + (size_t)cap + 3 * (size_t)cap + 2 * (size_t)cap;
    HIPC(hipMalloc(&d_rec, words * 4));
    HIPC(hipMemsetAsync(d_rec, 0, 16, own_stream(h)));
    GArgs A = gargs(h);
    A.emit_sel = idx % 64; A.emit_group = idx / 64; A.emit_w0 = 0; A.emit_wn = (uint32_t)E.total; A.emit_out = nullptr; A.emit_sites = d_rec; A.emit_sites_cap = cap;
    emit_units(h, A, EMIT_ALL_UNITS, launch_g_emit);
    HIPC(hipGetLastError());
    std::vector<uint32_t> rec(words);
    HIPC(hipMemcpyAsync(rec.data(), d_rec, words * 4, hipMemcpyDeviceToHost, own_stream(h)));
    HIPC(hipStreamSynchronize(own_stream(h)));
    HIPC(hipFree(d_rec));
    if (rec[0] > cap || rec[1] > cap || rec[2] > cap) { h->err = "internal: more self-check sites than derived wires"; return POB_E_STATE; }
    E.sc.z.assign(rec.begin() + 4, rec.begin() + 4 + rec[0]);
    std::sort(E.sc.z.begin(), E.sc.z.end(), [](uint32_t a, uint32_t b) { return (a & 0x7FFFFFFFu) < (b & 0x7FFFFFFFu); });
    std::vector<std::array<uint32_t, 3>> ms(rec[1]);
    for (uint32_t i = 0; i < rec[1]; i++) for (int j = 0; j < 3; j++) ms[i][j] = rec[4 + (size_t)cap + 3 * (size_t)i + j];
    std::sort(ms.begin(), ms.end());
    E.sc_ms = ms;
    std::vector<std::array<uint32_t, 2>> cs(rec[2]);
    for (uint32_t i = 0; i < rec[2]; i++) for (int j = 0; j < 2; j++) cs[i][j] = rec[4 + 4 * (size_t)cap + 2 * (size_t)i + j];
    std::sort(cs.begin(), cs.end());
    E.sc_cs = cs;
    HIPC(E.sc.upload(ms, cs));
    HIPC(hipMalloc(&E.d_sc_res, 16));
    E.sc_built = true;
    return POB_OK;
}
// ... and the reduced form's lists for the current map (E.map_id) and alias (pob_emit_selfcheck_alias)
static int sc_reduced_lists(pob_ctx* h) {
    EmitState& E = h->em;
    // the sites of this map: every wire through its class representative (pob_emit_selfcheck_alias; without one a wire stands for itself), a site with a wire
    // that is pinned to a constant or not kept is left out and counted; a copy site is a tautology between class members: counted as skipped
    const bool have_alias = E.sc_alias && E.sc_alias_n == h->plan.total.w;
    auto rep = [&](uint32_t w, uint32_t* out, bool may_be_const = true) -> bool {
        int64_t r = w;
        if (have_alias) {
            r = E.sc_alias[w];
            if (r < 0) {                                 // pinned to a constant: -1 - c for c < 2^30, INT32_MIN for a constant that does not fit
                if (!may_be_const || r == INT32_MIN) return false;
                *out = 0x80000000u | (uint32_t)(-1 - r); return true;
            }
        }
        if (!std::binary_search(E.keep.begin(), E.keep.end(), (uint32_t)r)) return false;
        *out = (uint32_t)r; return true;
    };
    std::vector<uint32_t> zr, mr; uint64_t left_out = E.sc_cs.size();
    for (uint32_t s0 : E.sc.z) {
        const uint32_t w = s0 & 0x7FFFFFFFu; uint32_t q[6] = {0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        bool ok = rep(w, &q[0], false) && rep(w + 1, &q[1]) && rep(w + 2, &q[2]);
        if (ok && (s0 >> 31)) ok = rep(w - 3, &q[3]) && rep(w - 2, &q[4]) && rep(w - 1, &q[5]);
        if (!ok) { left_out++; continue; }
        zr.insert(zr.end(), q, q + 6);
    }
    for (const std::array<uint32_t, 3>& m3 : E.sc_ms) {
        uint32_t q[4] = {0, 0, 0, m3[2]};
        if (!(rep(m3[0], &q[0], false) && rep(m3[0] - 1, &q[1], false) && rep(m3[1], &q[2], false))) { left_out++; continue; }
        mr.insert(mr.end(), q, q + 4);
    }
    if (E.d_sc_zr) { HIPC(hipFree(E.d_sc_zr)); E.d_sc_zr = nullptr; }
    if (E.d_sc_mr) { HIPC(hipFree(E.d_sc_mr)); E.d_sc_mr = nullptr; }
    HIPC(hipMalloc(&E.d_sc_zr, std::max<size_t>(zr.size(), 1) * 4)); HIPC(hipMalloc(&E.d_sc_mr, std::max<size_t>(mr.size(), 1) * 4));
    if (!zr.empty()) HIPC(hipMemcpy(E.d_sc_zr, zr.data(), zr.size() * 4, hipMemcpyHostToDevice));
    if (!mr.empty()) HIPC(hipMemcpy(E.d_sc_mr, mr.data(), mr.size() * 4, hipMemcpyHostToDevice));
    E.sc_red_nz = (uint32_t)(zr.size() / 6); E.sc_red_nm = (uint32_t)(mr.size() / 4); E.sc_red_host_skipped = left_out; E.sc_red_map = E.map_id;
    E.sc_zr_host.swap(zr); E.sc_mr_host.swap(mr); E.sc_red_have = true;
    return POB_OK;
}
// ... and the O0 tables of the GROUP check.  In the O0 form the Keccak runs' whole 64-wire blocks go straight into the tag planes: the group's scratch is never filled there
// and holds stale bytes.  Every site wire is a G unit's and E.runs are the Keccak kernels' wires, so no site should have a wire in a run; one that has is left out here
// (it counts as skipped) -- the kernels never read a position that the window's fill did not cover.  (E.runs: emit_streams_and_runs.)
static int gsc_build_tables(pob_ctx* h) {
    EmitState& E = h->em;
    auto in_run = [&](uint32_t w) {
        auto it = std::upper_bound(E.runs.begin(), E.runs.end(), w, [](uint32_t v, const EmitState::Run& r) { return v < r.w; });
        return it != E.runs.begin() && w - (it - 1)->w < (it - 1)->n;
    };
    std::vector<std::array<uint32_t, 3>> ms; std::vector<std::array<uint32_t, 2>> cs;
    E.gsc.z.clear(); E.gsc_in_runs = 0;
    for (uint32_t s0 : E.sc.z) {
        const uint32_t w = s0 & 0x7FFFFFFFu;
        bool hit = in_run(w) || in_run(w + 1) || in_run(w + 2);
        if (s0 >> 31) hit = hit || in_run(w - 3) || in_run(w - 2) || in_run(w - 1);
        if (hit) E.gsc_in_runs++; else E.gsc.z.push_back(s0);
    }
    for (const std::array<uint32_t, 3>& m3 : E.sc_ms) { if (in_run(m3[0]) || in_run(m3[0] - 1) || in_run(m3[1])) E.gsc_in_runs++; else ms.push_back(m3); }
    for (const std::array<uint32_t, 2>& c2 : E.sc_cs) { if (in_run(c2[0]) || in_run(c2[1])) E.gsc_in_runs++; else cs.push_back(c2); }
    // (all or nothing: a failure frees what was allocated, so that the next checked begin starts over without a leak)
    if (E.gsc.upload(ms, cs) != hipSuccess || hipMalloc(&E.d_gsc_res, 66 * 4) != hipSuccess) {
        (void)hipGetLastError();
        E.gsc.free(); if (E.d_gsc_res) { (void)hipFree(E.d_gsc_res); E.d_gsc_res = nullptr; }
        h->err = "group self-check: out of device memory for the site tables";
        return POB_E_NOMEM;
    }
    E.gsc_built = true;
    return POB_OK;
}

// common part of pob_emit_begin / pob_emit_begin_reduced: E.red / E.map_id / E.total are set
static int emit_start(pob_ctx* h, uint32_t idx, uint64_t window_wires) {
    EmitState& E = h->em;
    const int NS = EmitState::NSLOT;
    uint64_t nwin_ = 0;
    { int rc = emit_prepare(h, E.total, 8ull << 20, &window_wires, &nwin_); if (rc) return rc; }      // (default: 8 Mi wires = 256 MiB windows)
    {   // like the reference binary, no witness is written for an input that failed an assert (tests/test.py:65-68)
        const uint32_t st_w = E.status_host[idx];
        if (st_w != 0) { h->err = "witness " + std::to_string(idx) + " failed an assert (status " + std::to_string(st_w) + "): nothing to emit"; E.queued_idx = -1; E.pre_made = false; return POB_E_STATE; }
    }
    // the witness announced with pob_emit_queue, same payload and window size: its first window has been expanded (and is being copied)
    // behind the previous witness' last windows already -- continue from there, nothing to wait for
    if (E.pre_made && E.pre_made_gen == h->gen_count && E.queued_idx == (int64_t)idx && E.win_wires == window_wires && E.nwin == nwin_ && E.probe_map == E.map_id && E.pre_made_packed == E.packed) {
        E.first_slot = (E.first_slot + (uint32_t)E.nwin) % NS;
        E.idx = idx; E.next_make = 1; E.next_take = 0; E.active = true; E.queued_idx = -1; E.pre_made = false; E.grp.on = false;
        return POB_OK;
    }
    if (E.pre_made || E.queued_idx == (int64_t)idx) E.queued_idx = -1;      // (an announcement made BEFORE this begin, for the witness after this one, stays)
    E.pre_made = false;
    E.grp.on = false;
    { int rc = emit_streams_and_runs(h); if (rc) return rc; }
    if (E.alloc_wires < window_wires) {                                     // (re)allocated only when a larger window is asked for: K witnesses reuse the buffers
        for (int k = 0; k < NS; k++) {
            if (E.d_win[k]) { HIPC(hipFree(E.d_win[k])); E.d_win[k] = nullptr; }
            if (E.h_pin[k]) { HIPC(hipHostFree(E.h_pin[k])); E.h_pin[k] = nullptr; }
            HIPC(hipMalloc(&E.d_win[k], window_wires * 32));
            HIPC(hipHostMalloc((void**)&E.h_pin[k], window_wires * 32 + pack_fixed_bytes(window_wires) + 32, hipHostMallocDefault));      // (a packed window of nothing but wide values is that much longer than the canonical one)
        }
        E.alloc_wires = window_wires;
    }
    if (E.packed && E.pk_alloc_wires < E.alloc_wires) {                      // the packed form of a slot and the scan's scratch: with the first packed emission at a window size
        for (int k = 0; k < NS; k++) {
            if (E.d_pk[k]) { HIPC(hipFree(E.d_pk[k])); E.d_pk[k] = nullptr; }
            HIPC(hipMalloc(&E.d_pk[k], E.alloc_wires * 32 + pack_fixed_bytes(E.alloc_wires) + 32));
        }
        if (E.d_pk_blk) { HIPC(hipFree(E.d_pk_blk)); E.d_pk_blk = nullptr; }
        if (E.d_pk_tot) { HIPC(hipFree(E.d_pk_tot)); E.d_pk_tot = nullptr; }
        HIPC(hipMalloc(&E.d_pk_blk, ((E.alloc_wires + 63) / 64) * 4)); HIPC(hipMalloc(&E.d_pk_tot, ((E.alloc_wires + 4095) / 4096) * 4));
        if (!E.s_val) HIPC(hipStreamCreateWithPriority(&E.s_val, hipStreamNonBlocking, 0));
        E.pk_alloc_wires = E.alloc_wires;
    }
    { int rc = emit_probe_pass(h, idx / 64, window_wires, nwin_); if (rc) return rc; }
    if (E.sc_on && !E.sc_built) { int rc = sc_record_sites(h, idx); if (rc) return rc; }
    if (E.sc_on) {
        const uint32_t init[3] = {0xFFFFFFFFu, 0, 0};
        HIPC(hipMemcpyAsync(E.d_sc_res, init, 12, hipMemcpyHostToDevice, own_stream(h)));
        HIPC(hipStreamSynchronize(own_stream(h)));
        E.sc_checked = 0; E.sc_skipped = 0;
    }
    if (E.sc_on && E.red && E.sc_red_map != E.map_id) { int rc = sc_reduced_lists(h); if (rc) return rc; }
    for (int k = 0; k < NS; k++) HIPC(hipEventRecord(E.ev_free[k], E.s_copy));
    E.win_wires = window_wires; E.nwin = nwin_; E.idx = idx; E.next_make = 0; E.next_take = 0; E.first_slot = 0; E.active = true;
    for (; E.next_make < std::min<uint64_t>(1, E.nwin); E.next_make++) { int rc = emit_make_window(h, idx, E.next_make, (int)((E.first_slot + E.next_make) % NS)); if (rc) return rc; }
    return POB_OK;
}

static int emit_probe_pass(pob_ctx* h, uint32_t group, uint64_t window_wires, uint64_t nwin_) {
    EmitState& E = h->em;
    if ((E.probe_win != window_wires || E.probe_map != E.map_id) && nwin_ <= 64) {
        // probe pass: every G unit runs once with the emitter's stores replaced by "mark window position / window_wires"; a window then
        // launches only the units that can write into it (most windows hold nothing but Keccak round wires)
        const size_t nu = h->plan.units.size();
        if (!E.d_probe) HIPC(hipMalloc(&E.d_probe, nu * 8));
        HIPC(hipMemsetAsync(E.d_probe, 0, nu * 8, own_stream(h)));
        GArgs A = gargs(h);
        A.emit_sel = 0; A.emit_group = group; A.emit_w0 = 0; A.emit_wn = (uint32_t)window_wires; A.emit_probe = E.d_probe; A.emit_out = nullptr;
        if (E.red) { A.emit_rbits = E.d_rbits; A.emit_rpre = E.d_rpre; }
        emit_units(h, A, EMIT_ALL_UNITS, launch_g_emit);
        HIPC(hipGetLastError());
        std::vector<unsigned long long> mask(nu);
        HIPC(hipMemcpyAsync(mask.data(), E.d_probe, nu * 8, hipMemcpyDeviceToHost, own_stream(h)));
        HIPC(hipStreamSynchronize(own_stream(h)));
        std::vector<uint32_t> order;
        E.wsegs.assign(nwin_, {});
        for (uint64_t wi = 0; wi < nwin_; wi++)
            for (const pob_ctx::Seg& sg : h->emit_segs) {
                EmitState::WSeg ws{sg.lds, (uint32_t)order.size(), 0};
                for (uint32_t j = 0; j < sg.count; j++) { const uint32_t u = h->order[sg.first + j]; if ((mask[u] >> wi) & 1) order.push_back(u); }
                ws.count = (uint32_t)order.size() - ws.first;
                if (ws.count) E.wsegs[wi].push_back(ws);
            }
        if (E.d_order) { HIPC(hipFree(E.d_order)); E.d_order = nullptr; }
        HIPC(hipMalloc(&E.d_order, std::max<size_t>(order.size(), 1) * 4));
        if (!order.empty()) HIPC(hipMemcpy(E.d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice));
        E.probe_win = window_wires; E.probe_map = E.map_id;
    } else if (nwin_ > 64) { E.probe_win = 0; E.probe_map = E.map_id; }       // (too many windows for the probe's 64-bit masks: every unit runs for every window)
    return POB_OK;
}

int pob_emit_begin(pob_handle h, uint32_t idx, uint64_t window_wires) {
    if (!h) return POB_E_ARG;
    if (!h->generated || idx >= h->n) { h->err = "nothing generated / witness index out of range"; return POB_E_STATE; }
    HIPC(hipSetDevice(h->device));
    h->em.red = false; h->em.map_id = 0; h->em.total = h->plan.total.w; h->em.packed = false;
    return emit_start(h, idx, window_wires);
}

static int emit_begin_reduced(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, uint64_t window_wires, bool packed);
int pob_emit_begin_reduced(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, uint64_t window_wires) { return emit_begin_reduced(h, idx, keep, n_keep, window_wires, false); }
int pob_emit_begin_packed(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, uint64_t window_wires) {
    if (keep) return emit_begin_reduced(h, idx, keep, n_keep, window_wires, true);
    if (!h || n_keep) return POB_E_ARG;
    if (!h->generated || idx >= h->n) { h->err = "nothing generated / witness index out of range"; return POB_E_STATE; }
    HIPC(hipSetDevice(h->device));
    h->em.red = false; h->em.map_id = 0; h->em.total = h->plan.total.w; h->em.packed = true;
    return emit_start(h, idx, window_wires);
}

static int emit_set_map(pob_handle h, const uint32_t* keep, uint64_t n_keep);
static int emit_begin_reduced(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, uint64_t window_wires, bool packed) {
    if (!h || !keep || n_keep == 0) return POB_E_ARG;
    if (!h->generated || idx >= h->n) { h->err = "nothing generated / witness index out of range"; return POB_E_STATE; }
    HIPC(hipSetDevice(h->device));
    { int rc = emit_set_map(h, keep, n_keep); if (rc) return rc; }
    h->em.packed = packed;
    return emit_start(h, idx, window_wires);
}
// the reduced payload's map: validated, uploaded and made the current one (E.red / E.map_id / E.total); the same map again costs its hash, a pinned one nothing
static int emit_set_map(pob_handle h, const uint32_t* keep, uint64_t n_keep) {
    EmitState& E = h->em;
    const uint64_t W = h->plan.total.w;
    // a map the caller PINNED (pob_reduced_map_pin: same address and length, contents promised unchanged) is not hashed again; any other map is
    // hashed in full every time (86 MB / 9 ms for the production map): an address can be recycled for a different map of the same length
    const bool pinned = E.pin_id && keep == E.pin_ptr && n_keep == E.pin_n;
    const uint64_t id = pinned ? E.pin_id : (fnv64(keep, n_keep * 4) ^ (n_keep << 1));
    if (id != E.map_id || E.keep.size() != n_keep) {
        // a new map: validate (wire 0 first, strictly increasing, inside the circuit), build the bitmap and the per-word ranks, upload
        if (keep[0] != 0 || keep[n_keep - 1] >= W) { h->err = "reduced map: keep[0] must be wire 0 and every index must be < nWitness"; return POB_E_ARG; }
        const uint64_t nwords = (W + 63) / 64;
        std::vector<unsigned long long> bits(nwords, 0); std::vector<uint32_t> pre(nwords, 0);
        for (uint64_t i = 0; i < n_keep; i++) {
            if (i && keep[i] <= keep[i - 1]) { h->err = "reduced map: wire indices must be strictly increasing"; return POB_E_ARG; }
            if (keep[i] >= W) { h->err = "reduced map: every index must be < nWitness"; return POB_E_ARG; }      // (before bits[] is touched)
            bits[keep[i] >> 6] |= 1ull << (keep[i] & 63);
        }
        uint32_t acc = 0;
        for (uint64_t i = 0; i < nwords; i++) { pre[i] = acc; acc += (uint32_t)__builtin_popcountll(bits[i]); }
        if (E.s_copy) HIPC(hipStreamSynchronize(E.s_copy));
        HIPC(hipStreamSynchronize(own_stream(h)));
        if (E.d_rbits) { HIPC(hipFree(E.d_rbits)); E.d_rbits = nullptr; }
        if (E.d_rpre) { HIPC(hipFree(E.d_rpre)); E.d_rpre = nullptr; }
        HIPC(hipMalloc(&E.d_rbits, nwords * 8)); HIPC(hipMalloc(&E.d_rpre, nwords * 4));
        HIPC(hipMemcpy(E.d_rbits, bits.data(), nwords * 8, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(E.d_rpre, pre.data(), nwords * 4, hipMemcpyHostToDevice));
        E.keep.assign(keep, keep + n_keep);
        E.queued_idx = -1; E.pre_made = false;
    }
    E.red = true; E.map_id = id; E.total = n_keep;
    return POB_OK;
}

int pob_reduced_map_pin(pob_handle h, const uint32_t* keep, uint64_t n_keep) {
    if (!h) return POB_E_ARG;
    EmitState& E = h->em;
    if (!keep || n_keep == 0) { E.pin_ptr = nullptr; E.pin_n = 0; E.pin_id = 0; return POB_OK; }     // unpin
    E.pin_ptr = keep; E.pin_n = n_keep; E.pin_id = fnv64(keep, n_keep * 4) ^ (n_keep << 1);
    return POB_OK;
}

// the two counts of a packed window's header (values of 32 bits | wider ones) -> cnt; false, with h->err set, if they name more values than the window has wires
static bool packed_counts_ok(const uint8_t* hdr, uint64_t wn, pob_ctx* h, uint32_t cnt[2]) {
    memcpy(cnt, hdr + 20, 8);
    if ((uint64_t)cnt[0] + cnt[1] > wn) { h->err = "internal: packed window counts more values than wires"; return false; }
    return true;
}
static int emit_next(pob_handle h, bool packed, const uint8_t** data, uint64_t* bytes, uint64_t* first_wire, uint64_t* n_wires) {
    if (!h || !data || !first_wire || !n_wires) return POB_E_ARG;
    EmitState& E = h->em;
    if (!E.active) { h->err = "pob_emit_next without pob_emit_begin"; return POB_E_STATE; }
    if (E.grp.on) { h->err = "pob_emit_next / pob_emit_next_packed: the emission was begun with pob_emit_begin_group_packed"; return POB_E_STATE; }
    if (E.packed != packed) { h->err = packed ? "pob_emit_next_packed: the emission was not begun with pob_emit_begin_packed" : "pob_emit_next: the emission was begun with pob_emit_begin_packed"; return POB_E_STATE; }
    if (E.next_take == E.nwin) { E.active = false; *data = nullptr; *first_wire = E.total; *n_wires = 0; return POB_OK; }
    HIPC(hipSetDevice(h->device));
    const int NS = EmitState::NSLOT;
    // the window handed out by the previous call is released now.  Two windows beyond the one returned here are kept in the making: one is
    // being copied while the caller works on this one, the next one is being expanded
    while (E.next_make < E.nwin && E.next_make <= E.next_take + 2) {
        int rc = emit_make_window(h, E.idx, E.next_make, (int)((E.first_slot + E.next_make) % NS)); if (rc) return rc;
        E.next_make++;
    }
    // ... and when this witness has no more windows to make, the first window of the witness announced with pob_emit_queue
    if (E.next_make == E.nwin && E.nwin - E.next_take <= 2 && E.queued_idx >= 0 && !E.pre_made) {
        int rc = emit_make_window(h, (uint32_t)E.queued_idx, 0, (int)((E.first_slot + E.nwin) % NS)); if (rc) return rc;
        E.pre_made = true; E.pre_made_gen = h->gen_count; E.pre_made_packed = E.packed;
    }
    const uint64_t k = E.next_take++;
    const int slot = (int)((E.first_slot + k) % NS);
    HIPC(hipEventSynchronize(E.ev_copied[slot]));
    *data = E.h_pin[slot]; *first_wire = k * E.win_wires; *n_wires = std::min(E.win_wires, E.total - k * E.win_wires);
    if (packed) {             // the header is in pinned memory: its two counts give the length of the value sections, which cross now (a few MB)
        uint32_t cnt[2];
        if (!packed_counts_ok(E.h_pin[slot], *n_wires, h, cnt)) return POB_E_STATE;
        const uint64_t fixed = pack_fixed_bytes(*n_wires), vb = pack_value_bytes(cnt[0], cnt[1]);
        if (vb) {
            HIPC(hipMemcpyAsync(E.h_pin[slot] + fixed, E.d_pk[slot] + fixed, vb, hipMemcpyDeviceToHost, E.s_val));
            HIPC(hipStreamSynchronize(E.s_val));
            E.pk_d2h += vb;
        }
        if (bytes) *bytes = fixed + vb;
    }
    return POB_OK;
}
int pob_emit_next(pob_handle h, const uint8_t** data, uint64_t* first_wire, uint64_t* n_wires) { return emit_next(h, false, data, nullptr, first_wire, n_wires); }
int pob_emit_next_packed(pob_handle h, const uint8_t** data, uint64_t* bytes, uint64_t* first_wire, uint64_t* n_wires) {
    if (!bytes) return POB_E_ARG;
    return emit_next(h, true, data, bytes, first_wire, n_wires);
}

// ---- group emission: the packed windows of every selected witness of ONE group of 64 from a single pass over the resident vector (include/pob_hip.h).
// Per window: the Keccak runs' 64-wire blocks go straight into the 64 tag planes (k_emit_group.hip: transposition of the stored words, no canonical form), everything else
// -- the G units on EmitPT<true>, run edges, the whole reduced form -- into the group's canonical scratch, which the pack pass compacts with a witness dimension (k_pack.hip).
#define GROUP_DEFAULT_WINDOW (4ull << 20)
static int group_make_window(pob_ctx* h, uint64_t k) {
    EmitState& E = h->em; EmitGroup& Gr = E.grp;
    const int ps = (int)(k % 2);
    const uint64_t w0 = k * E.win_wires, wn = std::min(E.win_wires, E.total - w0);
    const uint32_t nblk = (uint32_t)((wn + 63) / 64);
    hipStream_t st = own_stream(h);
    HIPC(hipStreamWaitEvent(st, Gr.ev_free[ps], 0));                        // the copies of the window that used this packed slot before are done
    const u64* Gp = (const u64*)h->d_bits + (uint64_t)Gr.group * h->plan.bit_stride;
    const GroupWin GW{Gr.d_win, Gr.plane, Gr.lanes, (uint32_t)w0, (uint32_t)wn, E.red ? E.d_rbits : nullptr, E.red ? E.d_rpre : nullptr};
    struct Piece { const EmitState::Run* r; uint64_t lo, hi; };
    std::vector<Piece> canon;                                               // what of the runs takes the canonical route, launched behind the fill
    std::vector<std::pair<uint32_t, uint32_t>> ranges;                      // the block ranges of the window BETWEEN the direct ones: fill and pack pass run over these only
    uint32_t covered = 0;
    for_each_run_piece(E, w0, wn, [&](const EmitState::Run& r, uint64_t lo, uint64_t hi) {
        if (E.red) { canon.push_back({&r, lo, hi}); return; }
        // O0: the blocks of the window wholly inside the run go straight into the tag planes; the partial blocks at the run's ends (and at a window edge that is no multiple of 64) do not
        const uint64_t bA = (lo - w0 + 63) / 64, bB = (hi - w0) / 64;
        if (bB > bA) {
            const uint64_t wa = w0 + 64 * bA, wb = w0 + 64 * bB;
            if ((uint32_t)bA > covered) ranges.push_back({covered, (uint32_t)bA});
            covered = (uint32_t)bB;                                         // (the runs are sorted by wire and do not overlap)
            launch_k_emit_group_direct(Gp, Gr.d_pk[ps], Gr.pk_stride, Gr.lanes, (uint32_t)bA, (uint32_t)(bB - bA), AbsorbRef{r.b, r.prev, r.src},
                                       (r.absorb ? r.o : r.b) + (uint32_t)(wa - r.w), r.absorb ? h->d_ktab : nullptr, st);
            if (lo < wa) canon.push_back({&r, lo, wa});
            if (wb < hi) canon.push_back({&r, wb, hi});
        } else canon.push_back({&r, lo, hi});
    });
    if (covered < nblk) ranges.push_back({covered, nblk});
    const PackGroup PG{Gr.d_win, Gr.plane, Gr.d_pk[ps], Gr.pk_stride, Gr.lanes, Gr.d_blk, Gr.d_tot, Gr.d_hdr[ps]};
    launch_group_fill(PG, (uint32_t)wn, w0 == 0, ranges, st);               // 0xEE.. where no direct block is (a wire nobody owns is not a field element); wire 0 = 1 (always kept)
    GArgs A = gargs(h);
    A.emit_out = Gr.d_win; A.emit_plane = Gr.plane; A.emit_lanes = Gr.lanes; A.emit_sel = 0; A.emit_group = Gr.group; A.emit_w0 = (uint32_t)w0; A.emit_wn = (uint32_t)wn;
    if (E.red) { A.emit_rbits = E.d_rbits; A.emit_rpre = E.d_rpre; }
    emit_units(h, A, k, launch_g_emit_group);
    for (const Piece& c : canon) {
        const EmitState::Run& r = *c.r;
        launch_k_emit_group_canon(Gp, GW, (uint32_t)c.lo, AbsorbRef{r.b, r.prev, r.src}, (r.absorb ? r.o : r.b) + (uint32_t)(c.lo - r.w), (uint32_t)(c.hi - c.lo), r.absorb ? h->d_ktab : nullptr, st);
    }
    for (const EmitState::GXor& x : E.xor_now) {                        // test hook (pob_debug_group_emit_xor): behind the expansion, in front of the check
        if (!((Gr.lanes >> x.lane) & 1)) continue;
        uint64_t pos = x.wire;
        if (E.red) { const auto it = std::lower_bound(E.keep.begin(), E.keep.end(), x.wire); if (it == E.keep.end() || *it != x.wire) continue; pos = (uint64_t)(it - E.keep.begin()); }
        if (pos < w0 || pos >= w0 + wn) continue;
        launch_group_xor_byte(Gr.d_win + (uint64_t)x.lane * Gr.plane + (pos - w0) * 32 + x.byte, x.mask, st);
    }
    if (Gr.checked) {         // the derived wires' relations on the values just written into every selected witness' window: behind the scratch's last writer, in front of the pack pass
        const ScGroup SG{Gr.d_win, Gr.plane, Gr.lanes, (uint32_t)w0, (uint32_t)wn, E.red ? E.d_rbits : nullptr, E.red ? E.d_rpre : nullptr, E.d_gsc_res, E.d_gsc_res + 64};
        if (E.red) {          // every site whose wires are all kept (through their class representatives), at their ranks: the kernels find the window's own (lists: sc_reduced_lists)
            launch_selfcheck_group_zr(SG, E.d_sc_zr, E.sc_red_nz, st);
            launch_selfcheck_group_mr(SG, E.d_sc_mr, E.sc_red_nm, h->d_pow256, st);
        } else {              // sites by the wire range of the window, as emit_make_window selects them; the kernels skip (and count) a site one of whose wires is outside the window
            const SiteTables::Window S = E.gsc.window(w0, w0 + wn);
            launch_selfcheck_group_z(SG, S.z.p, S.z.n, st);
            launch_selfcheck_group_m(SG, S.m.p, S.m.n, h->d_pow256, st);
            launch_selfcheck_group_c(SG, S.c.p, S.c.n, st);
            E.gsc_launched += S.total();
        }
    }
    launch_pack_group(PG, w0, (uint32_t)wn, ranges, st);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(Gr.ev_made[ps], st));
    HIPC(hipStreamWaitEvent(E.s_copy, Gr.ev_made[ps], 0));
    HIPC(hipMemcpyAsync(Gr.h_hdr[ps], Gr.d_hdr[ps], (size_t)Gr.nsel * 32, hipMemcpyDeviceToHost, E.s_copy));     // the headers first: their counts size the windows' copies
    HIPC(hipEventRecord(Gr.ev_hdr[ps], E.s_copy));
    return POB_OK;
}

// the headers of window k are in pinned memory: lay the selected witnesses' windows out back to back in the pinned slot (grown to what the counts ask for) and copy them
static int group_copy_window(pob_ctx* h, uint64_t k) {
    EmitState& E = h->em; EmitGroup& Gr = E.grp;
    const int ps = (int)(k % 2), hs = (int)(k % 3);
    const uint64_t wn = std::min(E.win_wires, E.total - k * E.win_wires), fixed = pack_fixed_bytes(wn);
    HIPC(hipEventSynchronize(Gr.ev_hdr[ps]));
    uint64_t total = 0; uint32_t r = 0;
    for (uint32_t l = 0; l < 64; l++) {
        Gr.off[hs][l] = Gr.len[hs][l] = 0;
        if (!((Gr.lanes >> l) & 1)) continue;
        uint32_t cnt[2];
        if (!packed_counts_ok(Gr.h_hdr[ps] + 32 * (size_t)r++, wn, h, cnt)) return POB_E_STATE;
        Gr.off[hs][l] = total; Gr.len[hs][l] = fixed + pack_value_bytes(cnt[0], cnt[1]); total += Gr.len[hs][l];
    }
    if (Gr.pin_cap[hs] < total) {
        if (Gr.h_pin[hs]) { HIPC(hipHostFree(Gr.h_pin[hs])); Gr.h_pin[hs] = nullptr; Gr.pin_cap[hs] = 0; }
        const uint64_t cap = total + total / 8 + 4096;                     // (the windows of a payload differ in their values: some room, so that not every slightly longer one allocates)
        if (hipHostMalloc((void**)&Gr.h_pin[hs], cap, hipHostMallocDefault) != hipSuccess) { Gr.h_pin[hs] = nullptr; (void)hipGetLastError(); h->err = "group emission: out of pinned host memory"; E.active = false; return POB_E_NOMEM; }
        Gr.pin_cap[hs] = cap;
    }
    r = 0;
    for (uint32_t l = 0; l < 64; l++) {
        if (!Gr.len[hs][l]) continue;
        uint8_t* dst = Gr.h_pin[hs] + Gr.off[hs][l];
        memcpy(dst, Gr.h_hdr[ps] + 32 * (size_t)r++, 32);
        HIPC(hipMemcpyAsync(dst + 32, Gr.d_pk[ps] + (uint64_t)l * Gr.pk_stride + 32, Gr.len[hs][l] - 32, hipMemcpyDeviceToHost, E.s_copy));
    }
    E.pk_d2h += total;
    HIPC(hipEventRecord(Gr.ev_copied[hs], E.s_copy));
    HIPC(hipEventRecord(Gr.ev_free[ps], E.s_copy));
    return POB_OK;
}

int pob_emit_begin_group_packed(pob_handle h, uint32_t group, uint64_t lanes, const uint32_t* keep, uint64_t n_keep, uint64_t window_wires, uint64_t* lanes_out) {
    if (!h || !lanes_out || (!keep && n_keep) || (keep && !n_keep)) return POB_E_ARG;
    EmitState& E = h->em; EmitGroup& Gr = E.grp;
    if (!h->generated || (uint64_t)group * 64 >= h->n) { h->err = "nothing generated / group out of range"; return POB_E_STATE; }
    if (E.sc_on) { h->err = "pob_emit_selfcheck does not cover group emissions: switch it off and use pob_emit_group_selfcheck"; return POB_E_STATE; }
    for (const pob_ctx::Seg& sg : h->emit_segs) if (sg.lds == 5) { h->err = "group emission is for the circuits' mains, not for gadget-level mains"; return POB_E_STATE; }
    HIPC(hipSetDevice(h->device));
    uint64_t nwin_ = 0;
    { int rc = emit_prepare(h, keep ? n_keep : h->plan.total.w, GROUP_DEFAULT_WINDOW, &window_wires, &nwin_); if (rc) return rc; }      // (the payload's size: E.total once the map is set below)
    uint64_t good = 0;                                                      // the witnesses of the group that exist in this batch and passed every assert
    for (uint32_t l = 0; l < 64 && (uint64_t)group * 64 + l < h->n; l++) if (E.status_host[group * 64 + l] == 0) good |= 1ull << l;
    if (lanes & ~good) {
        const uint32_t l = (uint32_t)__builtin_ctzll(lanes & ~good);
        h->err = "group emission: witness " + std::to_string((uint64_t)group * 64 + l) + " is beyond the batch or failed an assert: nothing to emit";
        return POB_E_STATE;
    }
    if (!lanes) lanes = good;
    if (keep) { int rc = emit_set_map(h, keep, n_keep); if (rc) return rc; }
    else { E.red = false; E.map_id = 0; E.total = h->plan.total.w; }
    E.packed = true; E.queued_idx = -1; E.pre_made = false;                 // (a window pre-made for another kind of emission is not used, an announcement does not carry over)
    E.active = false;
    { int rc = emit_streams_and_runs(h); if (rc) return rc; }
    HIPC(hipStreamSynchronize(own_stream(h)));
    if (!Gr.ev_made[0]) {
        for (int k = 0; k < 2; k++) { HIPC(hipEventCreateWithFlags(&Gr.ev_made[k], hipEventDisableTiming)); HIPC(hipEventCreateWithFlags(&Gr.ev_hdr[k], hipEventDisableTiming)); HIPC(hipEventCreateWithFlags(&Gr.ev_free[k], hipEventDisableTiming)); }
        for (int k = 0; k < 3; k++) HIPC(hipEventCreateWithFlags(&Gr.ev_copied[k], hipEventDisableTiming));
    }
    if (lanes && Gr.alloc_wires < window_wires) {                           // device side, as a function of the window size w (include/pob_hip.h): 64 * 32 w scratch, 2 x 64 packed windows of any content, the scan's rows; nothing for an empty mask
        group_free_device(Gr);
        Gr.plane = window_wires * 32; Gr.pk_stride = window_wires * 32 + pack_fixed_bytes(window_wires) + 32;
        const uint64_t nblk = (window_wires + 63) / 64, nchunk = (window_wires + 4095) / 4096;
        bool ok = hipMalloc(&Gr.d_win, 64 * Gr.plane) == hipSuccess && hipMalloc(&Gr.d_blk, 64 * nblk * 4) == hipSuccess && hipMalloc(&Gr.d_tot, 64 * nchunk * 4) == hipSuccess;
        for (int k = 0; k < 2 && ok; k++)
            ok = hipMalloc(&Gr.d_pk[k], 64 * Gr.pk_stride) == hipSuccess && hipMalloc(&Gr.d_hdr[k], 64 * 32) == hipSuccess && hipHostMalloc((void**)&Gr.h_hdr[k], 64 * 32, hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            group_free_device(Gr);
            h->err = "group emission: out of device memory at this window size (about 6 177 bytes per window wire: pass a smaller window_wires)";
            return POB_E_NOMEM;
        }
        Gr.alloc_wires = window_wires;
    }
    if (lanes) { int rc = emit_probe_pass(h, group, window_wires, nwin_); if (rc) return rc; }
    if (E.gsc_on) {           // the group check: the handle's site tables (built by whichever switch needs them first), this map's lists, 64 verdict words and the two counters
        if (lanes) {
            if (!E.sc_built) { int rc = sc_record_sites(h, group * 64 + (uint32_t)__builtin_ctzll(lanes)); if (rc) return rc; }
            if (!E.gsc_built) { int rc = gsc_build_tables(h); if (rc) return rc; }
            if (E.red && E.sc_red_map != E.map_id) { int rc = sc_reduced_lists(h); if (rc) return rc; }
            uint32_t init[66]; for (int l = 0; l < 64; l++) init[l] = 0xFFFFFFFFu; init[64] = init[65] = 0;
            HIPC(hipMemcpyAsync(E.d_gsc_res, init, sizeof init, hipMemcpyHostToDevice, own_stream(h)));
            HIPC(hipStreamSynchronize(own_stream(h)));
        }
        E.gsc_have = false; E.gsc_lanes = lanes; E.gsc_red = E.red; E.gsc_launched = 0;
    }
    Gr.checked = E.gsc_on;
    E.xor_now.swap(E.xor_armed); E.xor_armed.clear();                       // (pob_debug_group_emit_xor: this emission only)
    Gr.on = true; Gr.group = group; Gr.lanes = lanes; Gr.nsel = (uint32_t)__builtin_popcountll(lanes); Gr.next_bulk = 0;
    *lanes_out = lanes;
    E.win_wires = window_wires; E.nwin = lanes ? nwin_ : 0; E.idx = group * 64; E.next_make = 0; E.next_take = 0; E.first_slot = 0; E.active = true;
    for (int k = 0; k < 2; k++) HIPC(hipEventRecord(Gr.ev_free[k], E.s_copy));
    if (E.nwin) { int rc = group_make_window(h, 0); if (rc) return rc; E.next_make = 1; }
    return POB_OK;
}

int pob_emit_next_group_packed(pob_handle h, const uint8_t* data[64], uint64_t bytes[64], uint64_t* first_wire, uint64_t* n_wires) {
    if (!h || !data || !bytes || !first_wire || !n_wires) return POB_E_ARG;
    EmitState& E = h->em; EmitGroup& Gr = E.grp;
    if (!E.active) { h->err = "pob_emit_next_group_packed without pob_emit_begin_group_packed"; return POB_E_STATE; }
    if (!Gr.on) { h->err = "pob_emit_next_group_packed: the emission was not begun with pob_emit_begin_group_packed"; return POB_E_STATE; }
    for (int l = 0; l < 64; l++) { data[l] = nullptr; bytes[l] = 0; }
    if (E.next_take == E.nwin) { E.active = false; if (Gr.checked) E.gsc_have = true; *first_wire = E.nwin ? E.total : 0; *n_wires = 0; return POB_OK; }
    HIPC(hipSetDevice(h->device));
    const uint64_t k = E.next_take;
    // the window handed out by the previous call is released now.  Window k + 1's headers have crossed (or are about to): its copies are queued behind window k's, and with
    // them in the queue its packed slot's successor, window k + 2, can be expanded -- k + 2 is expanded while k + 1 is copied and k is with the caller
    while (Gr.next_bulk < E.next_make && Gr.next_bulk <= k + 1) { int rc = group_copy_window(h, Gr.next_bulk); if (rc) return rc; Gr.next_bulk++; }
    while (E.next_make < E.nwin && E.next_make <= k + 2) {
        if (Gr.next_bulk + 2 <= E.next_make) break;                         // (the packed slot's previous window has no copies queued yet)
        int rc = group_make_window(h, E.next_make); if (rc) return rc;
        E.next_make++;
    }
    E.next_take++;
    const int hs = (int)(k % 3);
    HIPC(hipEventSynchronize(Gr.ev_copied[hs]));
    for (int l = 0; l < 64; l++) if (Gr.len[hs][l]) { data[l] = Gr.h_pin[hs] + Gr.off[hs][l]; bytes[l] = Gr.len[hs][l]; }
    *first_wire = k * E.win_wires; *n_wires = std::min(E.win_wires, E.total - k * E.win_wires);
    return POB_OK;
}

int pob_emit_selfcheck(pob_handle h, int enable) {
    if (!h) return POB_E_ARG;
    h->em.sc_on = enable != 0;
    h->em.queued_idx = -1; h->em.pre_made = false;       // (a window pre-made without the check is not part of a checked emission)
    return POB_OK;
}

int pob_emit_selfcheck_alias(pob_handle h, const int32_t* alias, uint64_t n_wires) {
    if (!h || (alias && n_wires != h->plan.total.w)) return POB_E_ARG;
    h->em.sc_alias = alias; h->em.sc_alias_n = alias ? n_wires : 0; h->em.sc_red_map = 0;       // (the lists of the next reduced emission are rebuilt)
    return POB_OK;
}

int pob_emit_selfcheck_result(pob_handle h, uint64_t* checked, uint64_t* skipped, uint32_t* first_bad_wire) {
    if (!h) return POB_E_ARG;
    EmitState& E = h->em;
    if (!E.sc_on || !E.sc_built) { h->err = "no self-checked emission yet (pob_emit_selfcheck, then an emission)"; return POB_E_STATE; }
    HIPC(hipSetDevice(h->device));
    HIPC(hipStreamSynchronize(own_stream(h)));
    uint32_t res[3];
    HIPC(hipMemcpy(res, E.d_sc_res, 12, hipMemcpyDeviceToHost));
    const uint64_t all = E.sc.size();
    const uint64_t done = E.red ? (uint64_t)res[2] : E.sc_checked - res[1];          // (reduced: the kernels count what they evaluate)
    if (checked) *checked = done;
    if (skipped) *skipped = all - done;
    if (first_bad_wire) *first_bad_wire = res[0];
    return POB_OK;
}

int pob_emit_group_selfcheck(pob_handle h, int enable) {
    if (!h) return POB_E_ARG;
    h->em.gsc_on = enable != 0;
    return POB_OK;
}

int pob_emit_group_selfcheck_result(pob_handle h, uint64_t* lanes, uint64_t* checked, uint64_t* skipped, uint32_t first_bad_wire[64]) {
    if (!h) return POB_E_ARG;
    EmitState& E = h->em;
    if (!E.gsc_have) { h->err = "no complete self-checked group emission (pob_emit_group_selfcheck, then a group emission read to n_wires = 0: windows are made ahead of the caller)"; return POB_E_STATE; }
    uint32_t res[66]; for (int l = 0; l < 64; l++) res[l] = 0xFFFFFFFFu; res[64] = res[65] = 0;
    uint64_t all = 0, done = 0;
    if (E.gsc_lanes) {
        HIPC(hipSetDevice(h->device));
        HIPC(hipStreamSynchronize(own_stream(h)));
        HIPC(hipMemcpy(res, E.d_gsc_res, sizeof res, hipMemcpyDeviceToHost));
        all = E.sc.size();
        done = E.gsc_red ? (uint64_t)res[65] : E.gsc_launched - res[64];      // (reduced: the kernels count what they evaluate; O0: what was launched less what they skipped)
    }
    if (lanes) *lanes = E.gsc_lanes;
    if (checked) *checked = done;
    if (skipped) *skipped = all - done;
    if (first_bad_wire) for (int l = 0; l < 64; l++) first_bad_wire[l] = ((E.gsc_lanes >> l) & 1) ? res[l] : 0xFFFFFFFFu;
    return POB_OK;
}

int pob_debug_selfcheck_sites(pob_handle h, int kind, uint32_t* out, uint64_t cap, uint64_t* n) {
    if (!h || !n || kind < 0 || kind > 4) return POB_E_ARG;
    EmitState& E = h->em;
    if (kind >= 3) {          // the reduced lists of the last checked reduced emission (either switch): as they are, nothing is built
        const std::vector<uint32_t>& v = kind == 3 ? E.sc_zr_host : E.sc_mr_host;
        if (!E.sc_red_have) { h->err = "no checked reduced emission yet"; return POB_E_STATE; }
        *n = v.size();
        if (out) { if (cap < v.size()) return POB_E_ARG; if (!v.empty()) memcpy(out, v.data(), v.size() * 4); }
        return POB_OK;
    }
    if (!E.sc_built) {
        if (!h->generated) { h->err = "nothing generated"; return POB_E_STATE; }
        HIPC(hipSetDevice(h->device));
        HIPC(hipEventSynchronize(h->ev_gen_done));
        if (h->evaluated) HIPC(hipEventSynchronize(h->ev_check_done));
        int rc = sc_record_sites(h, 0); if (rc) return rc;
    }
    const uint32_t* src = kind == 0 ? E.sc.z.data() : kind == 1 ? (const uint32_t*)E.sc_ms.data() : (const uint32_t*)E.sc_cs.data();
    const uint64_t words = kind == 0 ? E.sc.z.size() : kind == 1 ? 3 * E.sc_ms.size() : 2 * E.sc_cs.size();
    *n = words;
    if (out) {
        if (cap < words) return POB_E_ARG;
        if (words) memcpy(out, src, words * 4);
    }
    return POB_OK;
}

int pob_debug_group_emit_xor(pob_handle h, uint32_t lane, uint32_t wire, uint32_t byte, uint8_t mask) {
    if (!h || lane >= 64 || byte >= 32 || wire >= h->plan.total.w) return POB_E_ARG;
    if (h->em.xor_armed.size() >= 16) { h->err = "pob_debug_group_emit_xor: at most 16 entries per emission"; return POB_E_ARG; }
    h->em.xor_armed.push_back({lane, wire, byte, mask});
    return POB_OK;
}

int pob_emit_queue(pob_handle h, uint32_t next_idx) {
    if (!h) return POB_E_ARG;
    EmitState& E = h->em;
    if (!h->generated) { h->err = "nothing generated"; return POB_E_STATE; }
    if (next_idx >= h->n) { h->err = "witness index out of range"; return POB_E_STATE; }
    if (E.pre_made) return POB_OK;                      // (a first window is on its way already: one announcement at a time)
    if (E.sc_on) return POB_OK;                         // self-checked emissions are not overlapped: the check's result names ONE witness (pob_emit_selfcheck_result)
    HIPC(hipSetDevice(h->device));
    { int rc = emit_statuses(h); if (rc) return rc; }
    if (E.status_host[next_idx] != 0) { h->err = "witness " + std::to_string(next_idx) + " failed an assert: nothing to emit"; return POB_E_STATE; }
    E.queued_idx = next_idx;
    return POB_OK;
}

int pob_emit_witness(pob_handle h, uint32_t idx, uint8_t* dst, uint64_t cap) {
    if (!h || !dst) return POB_E_ARG;
    const uint64_t bytes = (uint64_t)h->plan.total.w * 32;
    if (cap < bytes) { h->err = "destination too small"; return POB_E_ARG; }
    int rc = pob_emit_begin(h, idx, 0);
    if (rc) return rc;
    for (;;) {
        const uint8_t* p; uint64_t w0, wn;
        rc = pob_emit_next(h, &p, &w0, &wn);
        if (rc) return rc;
        if (!wn) break;
        memcpy(dst + w0 * 32, p, wn * 32);
    }
    return POB_OK;
}

// iden3 .wtns container around the window stream ("wtns" v2, 2 sections: (1) n8 = 32, prime, nWitness  (2) values): the 76 bytes in front of the values of W wires
static void wtns_header(uint64_t W, uint8_t hdr[76]) {
    const uint64_t P64[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    uint32_t u32; uint64_t u64v;
    memcpy(hdr, "wtns", 4); u32 = 2; memcpy(hdr + 4, &u32, 4); memcpy(hdr + 8, &u32, 4);
    u32 = 1; memcpy(hdr + 12, &u32, 4); u64v = 40; memcpy(hdr + 16, &u64v, 8);
    u32 = 32; memcpy(hdr + 24, &u32, 4); memcpy(hdr + 28, P64, 32); u32 = (uint32_t)W; memcpy(hdr + 60, &u32, 4);
    u32 = 2; memcpy(hdr + 64, &u32, 4); u64v = W * 32; memcpy(hdr + 68, &u64v, 8);
}
// the file of the emission that has been begun
static int write_wtns_stream(pob_ctx* h, const char* path) {
    const uint64_t W = h->em.total;
    FILE* f = fopen(path, "wb");
    if (!f) { h->err = std::string("cannot open ") + path; h->em.active = false; return POB_E_IO; }
    uint8_t hdr[76]; wtns_header(W, hdr);
    bool ok = fwrite(hdr, 1, 76, f) == 76;
    uint8_t* canon = nullptr;                           // packed transfer: each window is expanded here on the host before it is written
    if (h->em.packed && !(canon = (uint8_t*)malloc(h->em.win_wires * 32))) { fclose(f); remove(path); h->em.active = false; h->err = "out of host memory"; return POB_E_NOMEM; }
    for (;;) {
        const uint8_t* p; uint64_t w0, wn, pb = 0;
        int rc = emit_next(h, h->em.packed, &p, &pb, &w0, &wn);
        if (!rc && wn && canon) { rc = pob_unpack_window(p, pb, canon, wn * 32, 0); if (rc) h->err = "internal: a packed window does not validate"; p = canon; }
        if (rc) { fclose(f); remove(path); free(canon); return rc; }
        if (!wn) break;
        if (ok) ok = fwrite(p, 1, wn * 32, f) == wn * 32;
    }
    free(canon);
    fclose(f);
    if (!ok) { remove(path); h->err = "write failed"; return POB_E_IO; }
    return POB_OK;
}
int pob_write_wtns(pob_handle h, uint32_t idx, const char* path) {
    if (!h || !path) return POB_E_ARG;
    int rc = pob_emit_begin(h, idx, 0);
    return rc ? rc : write_wtns_stream(h, path);
}
int pob_write_wtns_reduced(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, const char* path) {
    if (!h || !path) return POB_E_ARG;
    int rc = pob_emit_begin_reduced(h, idx, keep, n_keep, 0);
    return rc ? rc : write_wtns_stream(h, path);
}
int pob_write_wtns_packed(pob_handle h, uint32_t idx, const uint32_t* keep, uint64_t n_keep, const char* path) {
    if (!h || !path) return POB_E_ARG;
    int rc = pob_emit_begin_packed(h, idx, keep, n_keep, 0);
    return rc ? rc : write_wtns_stream(h, path);
}

// the .wtns files of every selected witness of a group: one group emission, each witness' windows expanded on the host (pob_unpack_window) into its own file
int pob_write_wtns_group(pob_handle h, uint32_t group, uint64_t lanes, const uint32_t* keep, uint64_t n_keep, const char* const paths[64]) {
    if (!h || !paths) return POB_E_ARG;
    uint64_t sel = 0;
    int rc = pob_emit_begin_group_packed(h, group, lanes, keep, n_keep, 0, &sel);
    if (rc) return rc;
    for (int l = 0; l < 64; l++) if (((sel >> l) & 1) && !paths[l]) { h->em.active = false; return POB_E_ARG; }
    const uint64_t W = h->em.total;
    FILE* f[64]; bool ok = true;
    for (int l = 0; l < 64; l++) f[l] = nullptr;
    uint8_t* canon = (uint8_t*)malloc(std::max<uint64_t>(h->em.win_wires, 1) * 32);
    auto fail = [&](int code, const std::string& msg) { for (int l = 0; l < 64; l++) if (f[l]) { fclose(f[l]); remove(paths[l]); } free(canon); h->em.active = false; if (!msg.empty()) h->err = msg; return code; };
    if (!canon) return fail(POB_E_NOMEM, "out of host memory");
    uint8_t hdr[76]; wtns_header(W, hdr);
    for (int l = 0; l < 64; l++) if ((sel >> l) & 1) {
        if (!(f[l] = fopen(paths[l], "wb"))) return fail(POB_E_IO, std::string("cannot open ") + paths[l]);
        ok = ok && fwrite(hdr, 1, 76, f[l]) == 76;
    }
    for (;;) {
        const uint8_t* p[64]; uint64_t pb[64], w0, wn;
        rc = pob_emit_next_group_packed(h, p, pb, &w0, &wn);
        if (rc) return fail(rc, "");
        if (!wn) break;
        for (int l = 0; l < 64; l++) if (p[l]) {
            if (pob_unpack_window(p[l], pb[l], canon, wn * 32, 0)) return fail(POB_E_STATE, "internal: a packed window does not validate");
            ok = ok && fwrite(canon, 1, wn * 32, f[l]) == wn * 32;
        }
    }
    for (int l = 0; l < 64; l++) if (f[l]) { ok = (fclose(f[l]) == 0) && ok; f[l] = nullptr; }
    free(canon);
    if (!ok) { for (int l = 0; l < 64; l++) if ((sel >> l) & 1) remove(paths[l]); h->err = "write failed"; return POB_E_IO; }
    return POB_OK;
}

// pob_emit_measure_packed per group: `count` groups from first_group, each with the mask `lanes` (0: every good witness); pass 1 takes the windows as they arrive in pinned memory,
// pass 2 also expands every witness' window into dst (one window's worth is enough); d2h_bytes = what pass 1 copied device-to-host
int pob_emit_measure_group(pob_handle h, uint32_t first_group, uint32_t count, uint64_t lanes, uint64_t window_wires, const uint32_t* keep, uint64_t n_keep, uint8_t* dst, uint64_t dst_cap, int threads,
                           double* seconds_pinned, double* seconds_expanded, uint64_t* d2h_bytes) {
    if (!h || !seconds_pinned || !d2h_bytes || count == 0 || threads < 0 || (dst && !seconds_expanded)) return POB_E_ARG;
    HIPC(hipSetDevice(h->device));
    for (int pass = 0; pass < (dst ? 2 : 1); pass++) {
        const uint64_t d0 = h->em.pk_d2h; volatile uint8_t sink = 0;
        timespec t0, t1; clock_gettime(CLOCK_MONOTONIC, &t0);
        for (uint32_t i = 0; i < count; i++) {
            uint64_t sel = 0;
            int rc = pob_emit_begin_group_packed(h, first_group + i, lanes, keep, n_keep, window_wires, &sel);
            if (rc) return rc;
            if (pass && dst_cap < h->em.win_wires * 32) { h->em.active = false; h->err = "destination smaller than a window"; return POB_E_ARG; }
            for (;;) {
                const uint8_t* p[64]; uint64_t pb[64], w0, wn;
                rc = pob_emit_next_group_packed(h, p, pb, &w0, &wn);
                if (rc) return rc;
                if (!wn) break;
                for (int l = 0; l < 64; l++) if (p[l]) {
                    sink = sink ^ p[l][0] ^ p[l][pb[l] - 1];
                    if (pass) { rc = pob_unpack_window(p[l], pb[l], dst, wn * 32, threads); if (rc) { h->em.active = false; h->err = "internal: a packed window does not validate"; return rc; } }
                }
            }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double sec = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
        if (pass) *seconds_expanded = sec; else { *seconds_pinned = sec; *d2h_bytes = h->em.pk_d2h - d0; }
    }
    return POB_OK;
}

// emission throughput: K witnesses back to back through the window pipeline, the windows only touched (first + last cache line).
// keep != NULL: the reduced form.  The buffers (two device windows, two pinned host windows, the probe tables) are set up by the
// first witness a handle emits at a window size: time a first call to see that cost, a second one for the steady state.
int pob_emit_measure_ex(pob_handle h, uint32_t first_idx, uint32_t count, uint64_t window_wires, const uint32_t* keep, uint64_t n_keep, double* seconds, uint64_t* bytes) {
    if (!h || !seconds || !bytes || count == 0) return POB_E_ARG;
    HIPC(hipSetDevice(h->device));
    uint64_t total = 0; volatile uint8_t sink = 0;
    timespec t0, t1; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint32_t i = 0; i < count; i++) {
        int rc = keep ? pob_emit_begin_reduced(h, first_idx + i, keep, n_keep, window_wires) : pob_emit_begin(h, first_idx + i, window_wires);
        if (rc) return rc;
        if (i + 1 < count) { rc = pob_emit_queue(h, first_idx + i + 1); if (rc) return rc; }
        for (;;) {
            const uint8_t* p; uint64_t w0, wn;
            rc = pob_emit_next(h, &p, &w0, &wn);
            if (rc) return rc;
            if (!wn) break;
            sink = sink ^ p[0] ^ p[wn * 32 - 1]; total += wn * 32;
        }
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    *seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec); *bytes = total;
    return POB_OK;
}
// the packed form: pass 1 takes the packed windows as they arrive in pinned memory, pass 2 also expands each into dst (the whole payload if it fits dst_cap, else every
// window at dst's start); d2h_bytes = what pass 1 copied device-to-host
int pob_emit_measure_packed(pob_handle h, uint32_t first_idx, uint32_t count, uint64_t window_wires, const uint32_t* keep, uint64_t n_keep, uint8_t* dst, uint64_t dst_cap, int threads,
                            double* seconds_pinned, double* seconds_expanded, uint64_t* d2h_bytes) {
    if (!h || !seconds_pinned || !d2h_bytes || count == 0 || threads < 0 || (dst && !seconds_expanded)) return POB_E_ARG;
    HIPC(hipSetDevice(h->device));
    for (int pass = 0; pass < (dst ? 2 : 1); pass++) {
        const uint64_t d0 = h->em.pk_d2h; volatile uint8_t sink = 0;
        timespec t0, t1; clock_gettime(CLOCK_MONOTONIC, &t0);
        for (uint32_t i = 0; i < count; i++) {
            int rc = pob_emit_begin_packed(h, first_idx + i, keep, n_keep, window_wires);
            if (rc) return rc;
            const bool whole = dst_cap >= h->em.total * 32;
            if (pass && !whole && dst_cap < h->em.win_wires * 32) { h->em.active = false; h->err = "destination smaller than a window"; return POB_E_ARG; }
            if (i + 1 < count) { rc = pob_emit_queue(h, first_idx + i + 1); if (rc) return rc; }
            for (;;) {
                const uint8_t* p; uint64_t pb, w0, wn;
                rc = pob_emit_next_packed(h, &p, &pb, &w0, &wn);
                if (rc) return rc;
                if (!wn) break;
                sink = sink ^ p[0] ^ p[pb - 1];
                if (pass) { rc = pob_unpack_window(p, pb, whole ? dst + w0 * 32 : dst, wn * 32, threads); if (rc) { h->em.active = false; h->err = "internal: a packed window does not validate"; return rc; } }
            }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double sec = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
        if (pass) *seconds_expanded = sec; else { *seconds_pinned = sec; *d2h_bytes = h->em.pk_d2h - d0; }
    }
    return POB_OK;
}
int pob_emit_measure(pob_handle h, uint32_t first_idx, uint32_t count, uint64_t window_wires, double* seconds, uint64_t* bytes) {
    return pob_emit_measure_ex(h, first_idx, count, window_wires, nullptr, 0, seconds, bytes);
}

// which inverse paths of the emitter have run since the last reset (policy.hpp EmitP::ctr); the emission must be complete (pob_emit_next returned its last window)
int pob_debug_emit_counters(pob_handle h, uint64_t out[4], int reset) {
    if (!h || !out) return POB_E_ARG;
    HIPC(hipSetDevice(h->device));
    uint32_t c[4];
    HIPC(hipStreamSynchronize(own_stream(h)));
    HIPC(hipMemcpy(c, h->d_emit_ctr, sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = c[k];
    if (reset) HIPC(hipMemset(h->d_emit_ctr, 0, sizeof c));
    return POB_OK;
}

}  // extern "C"
