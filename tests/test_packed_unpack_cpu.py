"""pob_unpack_window, the native host expansion of packed emission windows, against the numpy statement of the format (tests/packed_format.py).  No GPU is
touched and no shim is needed: the routine is host code of libpob_hip.so.  Under tools/run_sanitizers.py (POB_HOSTSIM_SAN=1) the same tests run against the
AddressSanitizer + UBSan build of the same source (tests/hostsim)."""
import ctypes
import os

import numpy as np
import pytest

from tests import packed_format as PF

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
E_ARG = -1
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    if os.environ.get("POB_HOSTSIM_SAN") == "1":
        from tests.hostsim import build as hb
        path = hb.build()
    else:
        import proof_of_burn_amd as pkg
        path = pkg.LIB_PATH
    so = ctypes.CDLL(path)
    so.pob_unpack_window.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
    return so


def _le(v: int) -> np.ndarray:
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


EDGES = [0, 1, 2, 2 ** 32 - 1, 2 ** 32, P - 1, 2 ** 256 - 1, int.from_bytes(b"\xEE" * 32, "little")]


def _values(n: int, seed: int) -> np.ndarray:
    """n canonical values: mostly 0 / 1 like a witness, runs of nothing but bits (the expansion's fast path), small and wide values, every edge value"""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 32), dtype=np.uint8)
    kind = rng.choice(4, size=n, p=[0.5, 0.44, 0.03, 0.03])
    v[kind == 1, 0] = 1
    sm = np.nonzero(kind == 2)[0]
    v[sm, :4] = rng.integers(0, 256, size=(sm.size, 4), dtype=np.uint8)
    wd = np.nonzero(kind == 3)[0]
    v[wd] = rng.integers(0, 256, size=(wd.size, 32), dtype=np.uint8)
    if n >= 1024:
        v[256:640] = 0
        v[256:640:3, 0] = 1
    at = rng.permutation(n)[:min(n, 4 * len(EDGES))]
    for k, i in enumerate(at):
        v[i] = _le(EDGES[(k + seed) % len(EDGES)])
    return v.ravel()


def _unpack(lib, packed: np.ndarray, n: int, threads: int, cap: int | None = None, misalign: int = 0):
    """-> (rc, destination [32 n], everything around it unchanged?)"""
    buf = np.full(32 * n + 2 * GUARD + 16, 0xA5, dtype=np.uint8)
    off = GUARD + (-(buf.ctypes.data + GUARD) % 16) + misalign
    packed = np.ascontiguousarray(packed)
    rc = lib.pob_unpack_window(packed.ctypes.data, packed.size, buf.ctypes.data + off, 32 * n if cap is None else cap, threads)
    guards_ok = bool((buf[:off] == 0xA5).all() and (buf[off + 32 * n:] == 0xA5).all())
    return rc, buf[off:off + 32 * n], guards_ok


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 300_007])
def test_unpack_window_round_trip(lib, n):
    vals = _values(n, seed=n)
    packed = PF.encode(vals, first_wire=7 * n)
    n_, ns, nw = PF.counts_of(vals)
    assert packed.size == PF.packed_size(n_, ns, nw) and (n < 64 or (ns and nw))
    fw, back = PF.decode(packed)
    assert fw == 7 * n and np.array_equal(back, vals)            # the helper agrees with itself
    for threads in (1, 0, 3):
        for misalign in (0, 4):                                      # 16-byte aligned destinations take the streaming stores, others the plain ones
            rc, got, guards_ok = _unpack(lib, packed, n, threads, misalign=misalign)
            assert rc == 0 and guards_ok, (n, threads, misalign, rc)
            assert np.array_equal(got, vals), (n, threads, misalign, int(np.nonzero(got != vals)[0][0]) // 32)


def test_unpack_window_all_kinds_alone(lib):
    """windows of one kind only: the counts' corners (no value section at all, nothing but wide values: the longest a packed window gets)"""
    n = 5000
    for edge in EDGES:
        vals = np.tile(_le(edge), n)
        packed = PF.encode(vals)
        rc, got, guards_ok = _unpack(lib, packed, n, 0)
        assert rc == 0 and guards_ok and np.array_equal(got, vals), hex(edge)
    assert PF.encode(np.tile(_le(P - 1), n)).size > 32 * n            # (which is why the handle's pinned slots have room for more than the canonical window)


def _malformed(n):
    vals = _values(n, seed=99)
    vals[-32:] = _le(P - 1)                                           # (the last wire is not 0: a header that claims one wire fewer leaves a tag bit beyond n)
    good = PF.encode(vals, first_wire=3)
    _, ns, nw = PF.counts_of(vals)
    o_planes, o_index, o_small, o_wide, total = PF.section_offsets(n, ns, nw)
    assert ns and nw
    cases = []
    for name, b in (("header", o_planes), ("planes", o_index), ("index", o_small), ("small", o_wide), ("wide", total)):
        if b < total:
            cases.append((f"truncated behind the {name}", good[:b]))
        cases.append((f"truncated one byte into the {name}", good[:b - 1]))
    cases.append(("one byte too long", np.concatenate([good, np.zeros(1, np.uint8)])))
    cases.append(("32 bytes too long", np.concatenate([good, np.zeros(32, np.uint8)])))

    def edit(name, off, delta, width=4):
        m = good.copy()
        x = int.from_bytes(m[off:off + width].tobytes(), "little") + delta
        m[off:off + width] = np.frombuffer((x % (1 << (8 * width))).to_bytes(width, "little"), dtype=np.uint8)
        cases.append((name, m))

    edit("wrong magic", 0, 1)
    edit("wrong version", 4, 1)
    edit("reserved word set", 28, 1)
    edit("n_wires - 1", 16, -1)
    edit("n_small + 1", 20, 1)
    edit("n_small - 1", 20, -1)
    edit("n_wide + 1", 24, 1)
    edit("n_wide - 1", 24, -1)
    nchunk = (n + 4095) // 4096
    edit("chunk index 0 small + 1", o_index, 1)
    edit("last chunk index small + 1", o_index + 8 * (nchunk - 1), 1)
    edit("last chunk index wide - 1", o_index + 8 * (nchunk - 1) + 4, -1)
    assert n % 64, "the case needs a partial last block"
    last = o_planes + 16 * ((n + 63) // 64 - 1)
    m = good.copy(); m[last + (n % 64) // 8] |= 1 << (n % 64 % 8); cases.append(("tag bit (lo) set beyond n", m))
    m = good.copy(); m[last + 8 + 7] |= 0x80; cases.append(("tag bit (hi) set beyond n", m))
    i0 = int(np.nonzero(PF.tags_of(vals) == 0)[0][0])
    m = good.copy(); m[o_planes + 16 * (i0 // 64) + 8 + (i0 % 64) // 8] |= 1 << (i0 % 8); cases.append(("a tag 0 turned into a small tag: popcount disagrees", m))
    m = good.copy(); m[o_small:o_small + 4] = 0; m[o_small] = 1; cases.append(("a small value below 2", m))
    m = good.copy(); m[o_wide + 4:o_wide + 32] = 0; cases.append(("a wide value that fits 32 bits", m))
    if o_wide - (o_small + 4 * ns):
        m = good.copy(); m[o_wide - 1] = 1; cases.append(("non-zero padding behind the small values", m))
    if o_small - (o_index + 8 * nchunk):
        m = good.copy(); m[o_small - 1] = 1; cases.append(("non-zero padding behind the chunk index", m))
    if o_index - (o_planes + 16 * ((n + 63) // 64)):
        m = good.copy(); m[o_index - 1] = 1; cases.append(("non-zero padding behind the tag planes", m))
    return good, cases


@pytest.mark.parametrize("n", [65, 4097 + 64 + 5, 40_000 + 7])
def test_unpack_window_refuses_malformed_windows_and_writes_nothing(lib, n):
    good, cases = _malformed(n)
    assert len(cases) >= 26
    rc, _, guards_ok = _unpack(lib, good, n, 1)
    assert rc == 0 and guards_ok
    for name, bad in cases:
        for threads in (1, 0):
            exact = np.array(bad, dtype=np.uint8, copy=True)          # (an exact-size copy: a read beyond the window is a heap overflow under AddressSanitizer)
            rc, dst, guards_ok = _unpack(lib, exact, n, threads)
            assert rc == E_ARG, (name, rc)
            assert guards_ok and (dst == 0xA5).all(), f"{name}: refused, but memory was written"
    # dst_cap one short
    for cap in (32 * n - 1, 32 * n - 32, 0):
        rc, dst, guards_ok = _unpack(lib, good, n, 0, cap=cap)
        assert rc == E_ARG and guards_ok and (dst == 0xA5).all(), cap
    assert lib.pob_unpack_window(None, 64, good.ctypes.data, 64, 0) == E_ARG and lib.pob_unpack_window(good.ctypes.data, good.size, None, 1 << 30, 0) == E_ARG
    assert lib.pob_unpack_window(good.ctypes.data, good.size, good.ctypes.data, 1 << 30, -1) == E_ARG


def test_python_mirror_unpack_window():
    from proof_of_burn_amd import witness as W
    vals = _values(10_000, seed=5)
    packed = PF.encode(vals, first_wire=123)
    assert np.array_equal(W.unpack_window(packed), vals) and np.array_equal(W.unpack_window(packed.tobytes()), vals)
    out = np.zeros(vals.size + 64, dtype=np.uint8)
    assert np.array_equal(W.unpack_window(packed, out), vals) and not out[vals.size:].any()
    with pytest.raises(ValueError):
        W.unpack_window(packed[:-1])
    with pytest.raises(ValueError):
        W.unpack_window(packed, np.zeros(vals.size - 1, dtype=np.uint8))
