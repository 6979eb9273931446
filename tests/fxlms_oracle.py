"""A numpy restatement of layered fixed-point min-sum (include/ldpc_hip.h, ldpc_fxlms_cfg): the
fxms front end, then integers only. Vectorised over the frames and row-serial in a given row
order. One pass (`trajectory`) keeps the decisions after every iteration, so the results for
every T up to the pass's and for early stop come from it (`result`). Besides the decoder's
results it reports the largest |app - c2v| before the message clamp, the largest |x + c| before
the APP clamp and how many values either clamp changed, so a test that claims "no saturation"
can assert its premise."""
import numpy as np

from fxms_oracle import GRID, MS, NMS, OMS, front, grid_samples, write_edge_code, write_regular_code  # noqa: F401
from ldpcsimulation_amd import codes

# The cases that tie the restatement (tests/test_fxlms_oracle.py) and the kernel
# (tests/test_fxlms.py) to the fp64 layered decoder: code, Eb/N0, T. On the grid of
# fxms_oracle.GRID 16-bit messages and APPs never saturate within these T (plain MS on the PEG
# code does by T = 10, so its T is a condition).
GRID_CASES = {"w1944": ("80211n_1944_r12.alist", 1.4, 10), "peg": ("PEGReg504x1008.alist", 2.0, 6)}

# LDS bounds of the kernel (fxlms.h kFxlmsMaxLds, kernels.h kMaxLds): one codeword's state, a workgroup
CW_LDS_BOUND, WG_LDS_BOUND = 64 * 1024, 160 * 1024


def cw_bytes(N, M, maxdc, app_bits):
    """LDS bytes of one codeword's state: N APPs, M sign words (two where a row has more than 26
    edges) and M magnitude pairs, each array padded to 16."""
    al = lambda x: (x + 15) & ~15
    wide = app_bits > 8
    return al(N * (2 if wide else 1)) + al(4 * M) * (2 if maxdc > 26 else 1) + al(M * (4 if wide else 2))


def sched_bytes(M, maxdc):
    """LDS bytes of the staged schedule: maxdc * M 16-bit bit indices and M degrees."""
    al = lambda x: (x + 15) & ~15
    return al(2 * max(maxdc, 1) * M) + al(M)


class Fxlms:
    def __init__(self, path):
        H = codes.read_alist(path)
        self.N, self.M = H.N, H.M
        self.rows = [np.array(r, dtype=np.int64) for r in H.rows]
        self.maxdc = max(len(r) for r in self.rows)
        self.E = sum(len(r) for r in self.rows)
        self._ecol = np.concatenate([r for r in self.rows if len(r)])
        deg = np.array([len(r) for r in self.rows])
        self._ptr = np.concatenate([[0], np.cumsum(deg)])[:-1][deg > 0]
        self._nz = deg > 0

    def syndrome_fail(self, dneg):
        """[B] bool: the decisions (True = bit 1) are not a codeword."""
        par = np.add.reduceat(dneg[:, self._ecol].astype(np.int32), self._ptr, axis=1) & 1
        return par.any(axis=1)

    def trajectory(self, Y, variant, T, msg_bits, app_bits, num=1, shift=0, beta=0, order=None):
        """T iterations over Y [B, N] integer codes, rows serially in `order` (None: 0..M-1).
        Returns a dict: dneg [T + 1, B, N] (the decisions after t iterations, True = bit 1), and per
        step t (0: the start, t: iteration t) and frame peak_x, peak_app and clamped [T + 1, B]."""
        Y = np.atleast_2d(np.asarray(Y)).astype(np.int32)
        B, V, A = Y.shape[0], (1 << (msg_bits - 1)) - 1, (1 << (app_bits - 1)) - 1
        order = range(self.M) if order is None else [int(j) for j in order]
        assert sorted(order) == list(range(self.M))
        app = np.clip(Y, -A, A)
        c2v = [np.zeros((B, len(r)), dtype=np.int32) for r in self.rows]
        dneg = np.empty((T + 1, B, self.N), dtype=bool)
        peak_x, peak_app, clamped = (np.zeros((T + 1, B), dtype=np.int64) for _ in range(3))
        peak_app[0], clamped[0] = np.abs(Y).max(axis=1), (np.abs(Y) > A).sum(axis=1)
        dneg[0] = app <= 0
        for t in range(1, T + 1):
            for j in order:
                b = self.rows[j]
                d = len(b)
                if d == 0:
                    continue
                pre = app[:, b] - c2v[j]
                x = np.clip(pre, -V, V)
                a, neg = np.abs(x), x < 0
                pos = a.argmin(axis=1)
                if d > 1:
                    part = np.partition(a, 1, axis=1)
                    m1, m2 = part[:, 0], part[:, 1]
                else:
                    m1, m2 = a[:, 0], np.full(B, V, dtype=np.int32)
                if variant == NMS:
                    m1, m2 = (m1 * num) >> shift, (m2 * num) >> shift
                elif variant == OMS:
                    m1, m2 = np.maximum(m1 - beta, 0), np.maximum(m2 - beta, 0)
                mag = np.where(np.arange(d)[None, :] == pos[:, None], m2[:, None], m1[:, None])
                flip = neg ^ ((neg.sum(axis=1) & 1) == 1)[:, None]
                c = np.where(flip, -mag, mag).astype(np.int32)
                post = x + c
                c2v[j] = c
                app[:, b] = np.clip(post, -A, A)
                np.maximum(peak_x[t], np.abs(pre).max(axis=1), out=peak_x[t])
                np.maximum(peak_app[t], np.abs(post).max(axis=1), out=peak_app[t])
                clamped[t] += (np.abs(pre) > V).sum(axis=1) + (np.abs(post) > A).sum(axis=1)
            dneg[t] = app <= 0
        return dict(dneg=dneg, peak_x=peak_x, peak_app=peak_app, clamped=clamped)

    def result(self, tr, T, early_stop=False, c=None):
        """The decoder's result at T <= the trajectory's: d [B, N] int8 bipolar, s [B] (the iteration
        whose decisions are returned), frames (bit_err, uncoded_bit_err, syndrome_fail, iters as the
        library reports them), and peak_x, peak_app, clamped over the iterations each frame ran."""
        dneg = tr["dneg"]
        B = dneg.shape[1]
        assert T < len(dneg)
        cneg = np.zeros((B, self.N), dtype=bool) if c is None else np.asarray(c).reshape(B, self.N) < 0
        s = np.full(B, T, dtype=np.int64)
        if early_stop:
            ok = np.stack([~self.syndrome_fail(dneg[t]) for t in range(T + 1)])   # [T + 1, B]
            s = np.where(ok.any(axis=0), ok.argmax(axis=0), T)
        out_d = dneg[s, np.arange(B)]
        ran = np.arange(len(dneg))[:, None] <= s[None, :]   # the start and iterations 1..s
        frames = np.zeros(B, dtype=[("bit_err", np.int32), ("uncoded_bit_err", np.int32), ("syndrome_fail", np.int32),
                                    ("iters", np.int32)])
        frames["bit_err"] = (out_d != cneg).sum(axis=1)
        frames["uncoded_bit_err"] = (dneg[0] != cneg).sum(axis=1)
        frames["syndrome_fail"] = self.syndrome_fail(out_d)
        frames["iters"] = s if early_stop else 0
        return dict(d=np.where(out_d, -1, 1).astype(np.int8), s=s, frames=frames,
                    peak_x=int(np.where(ran, tr["peak_x"], 0).max()), peak_app=int(np.where(ran, tr["peak_app"], 0).max()),
                    clamped=int(np.where(ran, tr["clamped"], 0).sum()))

    def decode(self, Y, variant, T, msg_bits, app_bits, num=1, shift=0, beta=0, early_stop=False, c=None, order=None):
        return self.result(self.trajectory(Y, variant, T, msg_bits, app_bits, num, shift, beta, order), T, early_stop, c)
