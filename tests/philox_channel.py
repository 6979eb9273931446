"""The on-device noise, restated in numpy: Philox4x32-10, the uniforms, Box-Muller, and the
counter layout of every stream the kernels draw (DESIGN.md §5a has the table).

    channel         counter (v // 4, lo32(cw), hi32(cw), stream_id), the four normals are bits
                    4 * (v // 4) .. + 3 of codeword number cw; y = c (1 + sigma n)
    EMS channel     counter (symbol, lo32(cw), hi32(cw), stream_id), the four normals are the
                    symbol's bits 0..3
    perturbation    counter (v // 4, c1, c2, (stream_id & 0xFFFFF) | (row + 1) << 20), times
                    noise_sigma; GDBF and RGDBF: (c1, c2) = the codeword number, row = the
                    iteration (RGDBF: phase * T + iteration); the every-attempt decoders:
                    (c1, c2) = (lo32(f), hi32(f) + attempt), row = the iteration
    NGDBFhw queue   counter (k // 4, lo32(cw), hi32(cw), (stream_id & 0xFFFFF) | 1 << 20), times
                    noise_sigma
    key             (lo32(seed), hi32(seed)) everywhere

The uniforms are the device's fp32 values bit for bit; the transform from them to the normals
is computed in float64, so what a kernel's hardware log / sqrt / sin / cos add is the only
difference between a device sample and this module's (tests/test_philox_channel.py bounds
it). No kernel text is used here: test_philox_channel pins philox() to the CPU oracle's
Philox, which test_oracle pins to the Random123 known answers."""
import math

import numpy as np

M32 = 0xFFFFFFFF
STREAM20 = 0xFFFFF          # the bits of stream_id the GDBF families keep in counter word 3
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK, _S32 = np.uint64(M32), np.uint64(32)


def lo32(x: int) -> int:
    return int(x) & M32


def hi32(x: int) -> int:
    return (int(x) >> 32) & M32


def _words(*xs):
    """Python ints or integer arrays as uint64 arrays of one shape, every value below 2^32."""
    arrs = [np.asarray(x, dtype=np.uint64) for x in xs]
    assert all(np.all(a <= _MASK) for a in arrs), "counter and key words are 32 bits wide"
    return np.broadcast_arrays(*arrs)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays of 32-bit words held in uint64:
    returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (a.copy() for a in _words(c0, c1, c2, c3, k0, k1))
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        ka = np.uint64((_W0 * r) & M32)
        kb = np.uint64((_W1 * r) & M32)
        n0 = (p1 >> _S32) ^ c1 ^ ((k0 + ka) & _MASK)
        n2 = (p0 >> _S32) ^ c3 ^ ((k1 + kb) & _MASK)
        c0, c1, c2, c3 = n0, p1 & _MASK, n2, p0 & _MASK
    return c0, c1, c2, c3


def uniforms(u):
    """The device's uniform of a Philox word, in fp32 and bit for bit: float32(u) * 2^-32 +
    2^-33, in (0, 1]. The conversion rounds to nearest even (u < 2^32 is exact in float64, so
    the one rounding is float64 -> float32); the product by 2^-32 is exact, so a fused
    multiply-add and a separate add give the same float."""
    f = np.asarray(u, dtype=np.uint64).astype(np.float64).astype(np.float32)
    return f * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def normals(u4):
    """Box-Muller on the four words of one Philox call, in float64 from the fp32 uniforms:
    n0, n1 = sqrt(-2 ln r1) (cos, sin)(2 pi a0) with a0 = uniforms(u0), r1 = uniforms(u1),
    and n2, n3 the same from (u2, u3). Returns an array with a last axis of 4."""
    out = []
    for ua, ur in ((u4[0], u4[1]), (u4[2], u4[3])):
        a = uniforms(ua).astype(np.float64)
        r = uniforms(ur).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(r))
        out += [rad * np.cos(2.0 * np.pi * a), rad * np.sin(2.0 * np.pi * a)]
    return np.stack(out, axis=-1)


def sigma_of(ebn0_db: float, R: float) -> float:
    """host_rt.h sim_point: N0 = 10^(-Eb/N0 / 10) / R, sigma = sqrt(N0 / 2), in double."""
    return math.sqrt(10.0 ** (-ebn0_db / 10.0) / R / 2.0)


def _groups(n):
    """Philox calls that cover n values, four per call."""
    return np.arange((n + 3) // 4, dtype=np.uint64)


def _frame_words(first_cw, batch):
    """Counter words 1 and 2 of frames first_cw .. first_cw + batch - 1, as columns."""
    cw = [int(first_cw) + b for b in range(batch)]
    assert cw[-1] < 1 << 64
    return (np.array([lo32(x) for x in cw], dtype=np.uint64)[:, None],
            np.array([hi32(x) for x in cw], dtype=np.uint64)[:, None])


def channel_noise(seed, stream_id, first_cw, batch, N):
    """The standard normals n[batch, N] of the channel of frames first_cw .. first_cw + batch - 1."""
    c1, c2 = _frame_words(first_cw, batch)
    u = philox(_groups(N)[None, :], c1, c2, stream_id, lo32(seed), hi32(seed))
    return normals(u).reshape(batch, -1)[:, :N]


def codeword_rows(first_cw, batch, cw_rows):
    """Row of a codeword table of cw_rows rows that frame b sends: (first_cw + b) % cw_rows,
    the sum in 64 bits."""
    return [((int(first_cw) + b) & ((1 << 64) - 1)) % cw_rows for b in range(batch)]


def channel(seed, stream_id, first_cw, batch, N, sigma, c=None):
    """y[batch, N] = c (1 + sigma n) in float64. c: None (all +1) or a bipolar codeword table
    [cw_rows, N], of which frame b sends row (first_cw + b) % cw_rows."""
    y = 1.0 + sigma * channel_noise(seed, stream_id, first_cw, batch, N)
    if c is not None:
        c = np.asarray(c)
        y = c[codeword_rows(first_cw, batch, len(c))] * y
    return y


def perturbation_word(stream_id, row):
    """Counter word 3 of perturbation row `row` (>= 0); at least 2^20, so no channel's word
    (stream_id < 2^20 in every family that draws perturbations)."""
    return (np.asarray(stream_id, dtype=np.uint64) & np.uint64(STREAM20)) | \
        ((np.asarray(row, dtype=np.uint64) + np.uint64(1)) << np.uint64(20))


def perturbation(seed, stream_id, c1, c2, row, N, noise_sigma):
    """Perturbation row(s) `row` (an int or an array of them) of counter words (c1, c2), times
    noise_sigma: [N] or [rows, N] in float64."""
    rows = np.atleast_1d(np.asarray(row, dtype=np.uint64))
    u = philox(_groups(N)[None, :], c1, c2, perturbation_word(stream_id, rows)[:, None], lo32(seed), hi32(seed))
    p = noise_sigma * normals(u).reshape(len(rows), -1)[:, :N]
    return p if np.ndim(row) else p[0]


def rstat_words(frame, attempt):
    """(c1, c2) of attempt `attempt` of frame number `frame` in the every-attempt decoders
    (rstat.hip): (lo32(f), hi32(f) + attempt)."""
    return lo32(frame), (hi32(frame) + int(attempt)) & M32


def ems_channel_noise(seed, stream_id, first_cw, batch, N):
    """GF(16): n[batch, 4 N]; symbol v's Philox call is counter word 0 = v and its four normals
    are the symbol's bits 0..3."""
    c1, c2 = _frame_words(first_cw, batch)
    u = philox(np.arange(N, dtype=np.uint64)[None, :], c1, c2, stream_id, lo32(seed), hi32(seed))
    return normals(u).reshape(batch, 4 * N)


def ems_channel(seed, stream_id, first_cw, batch, N, sigma):
    """y[batch, 4 N] of the all-zero codeword (every bit +1), in float64."""
    return 1.0 + sigma * ems_channel_noise(seed, stream_id, first_cw, batch, N)


def hw_queue(seed, stream_id, first_cw, batch, qlen, noise_sigma):
    """The NGDBFhw noise queue q[batch, qlen]: counter (k // 4, lo32(cw), hi32(cw),
    (stream_id & 0xFFFFF) | 1 << 20), times noise_sigma."""
    c1, c2 = _frame_words(first_cw, batch)
    u = philox(_groups(qlen)[None, :], c1, c2, int(perturbation_word(stream_id, 0)), lo32(seed), hi32(seed))
    return noise_sigma * normals(u).reshape(batch, -1)[:, :qlen]
