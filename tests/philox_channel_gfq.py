"""The on-device EMS channel of a GF(q) code with m = log2 q bits per symbol, restated in numpy
beside tests/philox_channel.py (its philox and normals): symbol v makes one Philox call, counter
(v, lo32(cw), hi32(cw), stream_id), key (lo32(seed), hi32(seed)); the call's first m normals are
the symbol's bits 0..m-1 and the others are dropped. m = 4 is philox_channel.ems_channel_noise."""
import numpy as np

import philox_channel as P


def ems_channel_noise(seed, stream_id, first_cw, batch, N, m):
    """n[batch, m N] of frames first_cw .. first_cw + batch - 1."""
    assert 1 <= m <= 4
    c1, c2 = P._frame_words(first_cw, batch)
    u = P.philox(np.arange(N, dtype=np.uint64)[None, :], c1, c2, stream_id, P.lo32(seed), P.hi32(seed))
    return np.ascontiguousarray(P.normals(u)[:, :, :m]).reshape(batch, m * N)
