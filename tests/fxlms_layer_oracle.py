"""The numpy restatement of layered fixed-point min-sum (tests/fxlms_oracle.py), a layer at a
time: rows of a layer share no bit, so all of them are updated at once (grouped by degree), where
fxlms_oracle.Fxlms.trajectory takes them one by one -- 1.6 s an iteration on DVB-S2 N=64800 for
four frames. `trajectory` returns what the row-serial one returns (the decisions after every
iteration, peak_x, peak_app and clamped per iteration and frame) and the APPs after the last
iteration, so Fxlms.result works on it. tests/test_fxlms_wg_host.py pins it to the row-serial
restatement in the same order."""
import numpy as np

import fxlms_oracle as FL


class LayerFxlms(FL.Fxlms):
    def layer_groups(self, order, ptr):
        """Per layer of (order, ptr), as Graph.layers() returns them: the bits of its rows of each
        degree > 0, [rows, degree]."""
        order, ptr = [int(j) for j in order], [int(p) for p in ptr]
        assert sorted(order) == list(range(self.M)) and ptr[0] == 0 and ptr[-1] == self.M
        layers = []
        for l in range(len(ptr) - 1):
            by_deg = {}
            for j in order[ptr[l]:ptr[l + 1]]:
                if len(self.rows[j]):
                    by_deg.setdefault(len(self.rows[j]), []).append(self.rows[j])
            groups = [np.array(by_deg[d], dtype=np.int64) for d in sorted(by_deg)]
            bits = np.concatenate([g.ravel() for g in groups]) if groups else np.zeros(0, dtype=np.int64)
            assert len(np.unique(bits)) == len(bits), "rows of layer %d share a bit" % l
            layers.append(groups)
        return layers

    def trajectory(self, Y, variant, T, msg_bits, app_bits, num=1, shift=0, beta=0, order=None, ptr=None):
        """Fxlms.trajectory in the row order `order`, whose layers `ptr` bounds; also returns
        app [B, N], the APPs after iteration T."""
        Y = np.atleast_2d(np.asarray(Y)).astype(np.int32)
        B, V, A = Y.shape[0], (1 << (msg_bits - 1)) - 1, (1 << (app_bits - 1)) - 1
        layers = self.layer_groups(order, ptr)
        app = np.clip(Y, -A, A)
        c2v = [[np.zeros((B,) + g.shape, dtype=np.int32) for g in groups] for groups in layers]
        dneg = np.empty((T + 1, B, self.N), dtype=bool)
        peak_x, peak_app, clamped = (np.zeros((T + 1, B), dtype=np.int64) for _ in range(3))
        peak_app[0], clamped[0] = np.abs(Y).max(axis=1), (np.abs(Y) > A).sum(axis=1)
        dneg[0] = app <= 0
        for t in range(1, T + 1):
            for groups, msgs in zip(layers, c2v):
                for k, g in enumerate(groups):
                    d = g.shape[1]
                    pre = app[:, g] - msgs[k]                      # [B, rows, d]
                    x = np.clip(pre, -V, V)
                    a, neg = np.abs(x), x < 0
                    pos = a.argmin(axis=2)
                    if d > 1:
                        part = np.partition(a, 1, axis=2)
                        m1, m2 = part[:, :, 0], part[:, :, 1]
                    else:
                        m1, m2 = a[:, :, 0], np.full(a.shape[:2], V, dtype=np.int32)
                    if variant == FL.NMS:
                        m1, m2 = (m1 * num) >> shift, (m2 * num) >> shift
                    elif variant == FL.OMS:
                        m1, m2 = np.maximum(m1 - beta, 0), np.maximum(m2 - beta, 0)
                    mag = np.where(np.arange(d)[None, None, :] == pos[:, :, None], m2[:, :, None], m1[:, :, None])
                    flip = neg ^ ((neg.sum(axis=2) & 1) == 1)[:, :, None]
                    c = np.where(flip, -mag, mag).astype(np.int32)
                    post = x + c
                    msgs[k] = c
                    app[:, g] = np.clip(post, -A, A)
                    np.maximum(peak_x[t], np.abs(pre).max(axis=(1, 2)), out=peak_x[t])
                    np.maximum(peak_app[t], np.abs(post).max(axis=(1, 2)), out=peak_app[t])
                    clamped[t] += (np.abs(pre) > V).sum(axis=(1, 2)) + (np.abs(post) > A).sum(axis=(1, 2))
            dneg[t] = app <= 0
        return dict(dneg=dneg, peak_x=peak_x, peak_app=peak_app, clamped=clamped, app=app)
