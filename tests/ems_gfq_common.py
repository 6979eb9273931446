"""Shared by the GF(4) / GF(8) EMS tests: the small codes, the frames and the comparison with the
CPU oracle (oracle/ems_oracle.c), computed once per (code, frames, configuration)."""
import functools
import math

import numpy as np

from oracle import oracle as O

QS = (4, 8)
# (N, M, dv): row degree 4 (the DC = 4 build); row degree 6 (DC = 8); row degrees 4 and 5 with
# column degree 3 (beyond the symbol node's two-edge register cache); more symbols than any block
# has threads, maxdc * M = 3000 padded to a 4096-slot stride
SHAPES = [(96, 48, 2), (120, 40, 2), (90, 60, 3), (1300, 600, 2)]


def ems_cfgs(q):
    return [dict(nm=q, offset=0.0, early_stop=True), dict(nm=q, offset=0.0, early_stop=False),
            dict(nm=q // 2, offset=0.5, early_stop=True), dict(nm=2, offset=1.0, early_stop=False)]


@functools.lru_cache(maxsize=None)
def peg_code(N, M, dv, q):
    from ldpcsimulation_amd import codes
    return codes.peg_nb_code(N, M, dv, q, seed=N + M + q)


def random_nb_code(col_deg, row_deg, q, seed):
    """A random GF(q) code with the given column and row degrees (sum equal; no edge twice), fast
    at any size (PEG is not)."""
    from ldpcsimulation_amd import codes
    rng = np.random.default_rng(seed)
    col_deg, row_deg = list(col_deg), list(row_deg)
    assert sum(col_deg) == sum(row_deg) and min(row_deg) >= 2
    N, M = len(col_deg), len(row_deg)
    rsock = np.repeat(np.arange(M), row_deg)
    for _ in range(1000):
        perm = rng.permutation(len(rsock))
        cols, at = [], 0
        for d in col_deg:
            cols.append(sorted(int(r) for r in rsock[perm[at:at + d]]))
            at += d
        if all(len(set(c)) == len(c) for c in cols):
            break
    else:
        raise RuntimeError("no simple graph found")
    cols = [[(c, int(rng.integers(1, q))) for c in r] for r in cols]
    rows = [[] for _ in range(M)]
    for v, r in enumerate(cols):
        for c, h in r:
            rows[c].append((v, h))
    return codes.NbParityCheck(N, M, q, rows, cols)


def frames(N, m, nframes, ebn0, seed, R, c=None):
    """BPSK per bit (bit i of the symbol value, 0 -> +1), y = x(1 + sigma n), float32: y[nframes, N m], N0."""
    rng = np.random.default_rng(seed)
    n0 = 10 ** (-ebn0 / 10) / R
    sigma = math.sqrt(n0 / 2)
    x = np.ones((nframes, N * m), dtype=np.float64)
    if c is not None:
        x = 1.0 - 2.0 * ((c[:, :, None] >> np.arange(m)) & 1).reshape(nframes, N * m)
    y = (x * (1 + sigma * rng.standard_normal((nframes, N * m)))).astype(np.float32)
    y.setflags(write=False)
    return y, n0


@functools.lru_cache(maxsize=None)
def small_case(N, M, dv, q):
    """(code, oracle, y, n0) of a small code: eight frames at 2.0 dB, frame seed N + q."""
    H = peg_code(N, M, dv, q)
    A = O.NbCode(H)
    y, n0 = frames(H.N, A.m, 8, 2.0, N + q, 1 - M / N)
    return H, A, y, n0


_WANT = {}


def oracle_decode(key, A, y, n0, T, **cfg):
    """A.decode, computed once per (key, T, cfg) and left unchanged."""
    k = (key, T, tuple(sorted(cfg.items())))
    if k not in _WANT:
        r = A.decode(y, n0, T, **cfg)
        for a in r:
            a.setflags(write=False)
        _WANT[k] = r
    return _WANT[k]


def bits_of(sym):
    """Set bits of every symbol, summed per frame."""
    return np.array([sum(bin(int(s)).count("1") for s in row) for row in sym])


def assert_equals_oracle(native, ctx, A, key, y, n0, T, cfg, c=None):
    """Decided symbols, iterations, syndrome flags, bit errors and the counters, as
    tests/test_ems.py::test_ems_decisions_bit_exact_vs_oracle; returns the oracle's (d, iters, fail)."""
    d, fr, cnt = ctx.decode(y, n0, native.EmsConfig(T=T, **cfg), c=c)
    want, its, sf = oracle_decode(key, A, y, n0, T, **cfg)
    assert int((d != want).sum()) == 0, f"{key} T={T} {cfg}: {(d != want).sum()} symbols differ"
    assert np.array_equal(fr["iters"], its) and np.array_equal(fr["syndrome_fail"], sf), (key, T, cfg)
    ref = want if c is None else want ^ c
    be = bits_of(ref)
    assert np.array_equal(fr["bit_err"], be), (key, T, cfg)
    assert cnt.frames == len(y) and cnt.iters == int(its.sum()) and cnt.bit_err == int(be.sum())
    assert cnt.symbol_err == int((ref != 0).sum()) and cnt.frame_err == int((ref != 0).any(axis=1).sum())
    assert cnt.syndrome_fail == int(sf.sum())
    return want, its, sf
