"""The device field arithmetic at its rare branches, without a GPU: the Python model of the device inversion (tests/fr_inv_model.py) against pow
over the edge inputs of tests/fr_edge_cases.py, with the conditions that make the set worth running (every branch, every shift width, both ends of
the k range); the inversion's table and the limb constants of fr_dev.hpp against Python; and the host build of the kernels (tests/hostsim), whose
k_fr_inv_test runs the device's own Kaliski body.  The device forms themselves (inline-asm product, the code the GPU compiler makes of the
inversion): tests/test_fr_edges_gpu.py, same inputs, same checks."""
import os
import re

import pytest

from tests import fr_edge_cases as E
from tests import fr_inv_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "proof_of_burn_amd", "csrc")
P = M.P


@pytest.fixture(scope="module")
def model_runs():
    """[(family, targets, waves)] -- the model over the whole set, computed once"""
    return [(name, xs, M.invert_all(xs)) for name, xs in E.inv_families()]


@pytest.fixture(scope="module")
def lib():
    from tests.hostsim import build as hb
    from proof_of_burn_amd import witness as W
    old = (W.LIB_PATH, W._lib)
    W.LIB_PATH, W._lib = hb.build(), None
    yield W.load_library()
    W.LIB_PATH, W._lib = old


def _lanes(model_runs):
    return [(x, lane) for _, xs, waves in model_runs for x, lane in zip(xs, (l for w in waves for l in w.lanes))]


def test_model_equals_pow_on_every_input(model_runs):
    assert M.R == 2 ** 256 % P and M.R * M.RINV % P == 1
    for x, lane in _lanes(model_runs):
        assert lane.result * M.RINV % P == pow(E.to_canonical(x), P - 2, P), hex(x)
    for call in E.inv_partial_calls():
        for x, lane in zip(call, (l for w in M.invert_all(call) for l in w.lanes)):
            assert lane.result * M.RINV % P == pow(E.to_canonical(x), P - 2, P), hex(x)


def test_input_set_reaches_every_branch_shift_width_and_both_ends_of_k(model_runs):
    """conditions on the SET (if one fails, the set is extended, not the condition): each branch counter >= 8, every batched shift width 1..31 run,
    k <= 260 and k >= 500 reached; and every k inside the table's rows that a result can select, [254, 508]"""
    lanes = _lanes(model_runs)
    steps = {c: sum(getattr(l, c) for _, l in lanes) for c in ("even_fix", "even_fix_w0_zero", "both_odd", "both_odd_d0_zero")}
    inputs = {c: sum(getattr(l, c) > 0 for _, l in lanes) for c in steps}
    widths = [sum(l.shifts[t] for _, l in lanes) for t in range(32)]
    ks = [l.k for x, l in lanes if x]
    print("steps per branch:", steps)
    print("inputs that reach each branch:", inputs, "of", len(ks), "non-zero inputs")
    print("steps per shift width 1..31:", widths[1:])
    print("k range:", min(ks), "..", max(ks))
    assert all(n >= 8 for n in steps.values()), steps
    assert all(n >= 8 for n in inputs.values()), inputs
    assert widths[0] == 0 and all(widths[t] >= 1 for t in range(1, 32)), widths
    assert min(ks) <= 260 and max(ks) >= 500, (min(ks), max(ks))
    assert 254 <= min(ks) and max(ks) <= 508, (min(ks), max(ks))


def test_every_wave_ends_within_the_loop_bound(model_runs):
    """the loop's own bound of 1 100 iterations is a silent fall-back: a wave it ended would write wrong wires with no status"""
    counts = {name: [w.iterations for w in waves] for name, _, waves in model_runs}
    for call in E.inv_partial_calls():
        counts["partial n=%d" % len(call)] = [w.iterations for w in M.invert_all(call)]
    print("loop iterations per wave:", counts)
    top = max(n for c in counts.values() for n in c)
    print("largest:", top, "of", M.LOOP_BOUND)
    assert top < M.LOOP_BOUND           # (the model itself asserts that no lane was still active)
    src = open(os.path.join(CSRC, "fr_dev.hpp")).read()
    body = src[src.index("HD Fr fr_inv_kaliski_inl"):]
    assert re.search(r"for \(int it = 0; it < (\d+); it\+\+\)", body).group(1) == str(M.LOOP_BOUND)


def _limbs(v):
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def parse_pow2_table(text):
    n = int(re.search(r"#define FR_POW2_TAB_LEN (\d+)", text).group(1))
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{8})u", text[text.index("FR_POW2_TAB_INIT"):])]
    return n, words


def check_pow2_table(text):
    n, words = parse_pow2_table(text)
    assert n == 521 == M.POW2_TAB_LEN and len(words) == 8 * n
    for k in range(n):
        assert words[8 * k:8 * k + 8] == _limbs(pow(2, 768 - k, P)), "row %d != 2^(768-%d) mod p" % (k, k)


def test_pow2_table_rows_equal_two_to_768_minus_k():
    check_pow2_table(open(os.path.join(CSRC, "fr_pow2_table.h")).read())


def test_a_flipped_limb_in_an_unvisited_table_row_is_caught():
    """row 300: below every k a random input produces (328..395 over thousands), so only the table check (and the edge inputs) can see it"""
    text = open(os.path.join(CSRC, "fr_pow2_table.h")).read()
    lines = text.split("\n")
    first = next(i for i, ln in enumerate(lines) if ln.startswith("    0x"))
    row = lines[first + 300]
    w = re.search(r"0x([0-9a-f]{8})u", row).group(1)
    lines[first + 300] = row.replace(w, "%08x" % (int(w, 16) ^ 0x100), 1)
    with pytest.raises(AssertionError, match="row 300"):
        check_pow2_table("\n".join(lines))


def _macro_limbs(src, name):
    body = re.search(r"#define %s\s+\{([^}]*)\}" % name, src).group(1)
    ws = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    assert len(ws) == 8
    return sum(w << (32 * j) for j, w in enumerate(ws))


def test_limb_constants_of_fr_dev():
    src = open(os.path.join(CSRC, "fr_dev.hpp")).read()
    assert _macro_limbs(src, "FR_P_LIMBS") == P
    assert _macro_limbs(src, "FR_R_LIMBS") == 2 ** 256 % P
    assert _macro_limbs(src, "FR_R2_LIMBS") == 2 ** 512 % P
    assert _macro_limbs(src, "FR_R3_LIMBS") == 2 ** 768 % P
    ninv = int(re.search(r"#define FR_NINV32 0x([0-9a-fA-F]+)u", src).group(1), 16)
    assert ninv == -pow(P, -1, 2 ** 32) % 2 ** 32
    fermat = src[src.index("HD Fr fr_inv_fermat(const Fr& a) {"):]
    ws = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)u", re.search(r"const uint32_t E\[8\] = \{([^}]*)\}", fermat).group(1))]
    assert len(ws) == 8 and sum(w << (32 * j) for j, w in enumerate(ws)) == P - 2
    assert re.search(r"for \(int i = (\d+); i >= 0; i--\)", fermat).group(1) == str((P - 2).bit_length() - 1)     # the ladder starts at the exponent's top bit


def test_crossed_operands_are_the_value_list_of_check_fr_sqr():
    """fr_edge_cases.fr_sqr_values restates the list check_fr_sqr builds for itself: a recording stand-in for the library sees what that check sends"""
    from tests.test_poseidon_lanes_cpu import check_fr_sqr

    class Recorder:
        def pob_debug_fr_sqr(self, device, buf, n, out_sqr, out_mul):
            self.sent = E._unpack(buf)
            return 1                            # the check stops at its first assert

    rec = Recorder()
    with pytest.raises(AssertionError):
        check_fr_sqr(rec)
    assert rec.sent == E.fr_sqr_values()


def test_host_build_inversions_on_the_edge_set(lib):
    """the host build of k_fr_inv_test: its first output is the device's Kaliski body (fr_inv_kaliski_inl, meeting per wavefront in the shim), its second the
    host's binary Euclid"""
    E.check_fr_inv(lib, E.inv_targets())
    for call in E.inv_partial_calls():
        E.check_fr_inv(lib, call)


def test_host_build_field_operations(lib):
    E.check_fr_ops(lib)
