"""Every kernel shape on codes whose check degree goes past 8.

The code fixtures have row degree <= 8, so of the instantiations the kernels are built in
-- k_decode_rows and k_rows_fast over (DC, CPT, RPT), the flood and layered kernels over DC,
the generic BP / GDBF / DD-BMP / RSMNGDBF kernels at any row degree -- the other tests
launch the two DC = 8 shapes (8, 2, 1) and (8, 4, 2) only. Here twelve tiny synthetic codes
(CODES; the generator of test_frame_tail with a column degree per bit) reach each of the
nine row-kernel shapes, the packed-state bound of the flood and layered kernels (row degree
26 / 27) and the bound of the BP check node and of the row schedule (32 / 33). Every test
asserts from kernel_info and row_sched_info the kernel and the shape it means to run, then
compares with the CPU oracle of the same operation: exact equality everywhere but the one
fp32 BP tolerance (test_bp.F32_BIT_TOL).

In each DC class a code has a row at the class's cap (8, 16, 32; at DC 8 and 16 in every
shape), one has its widest row at the least degree that selects the class (9, 17), one carries a degree-1 and a degree-2 row
(+-inf messages, then inf - inf = NaN) and N is off the multiples of 4 in two of the three:
126 leaves two bits and 1037 one bit in the last Philox group. The (DC, 4, 1) codes have
N = 252 on purpose, see test_on_device_channel."""
import functools

import numpy as np
import pytest

import ddbmp_oracle as D
import rgdbf_oracle as RO
from ldpcsimulation_amd import codes, native
from oracle import oracle as O
from test_bp import F32_BIT_TOL
from test_gpu_parity import VARIANTS as PARITY_VARIANTS
from test_gpu_parity import _oracle_front

pytestmark = pytest.mark.gpu

# name -> (N, M, ((bits, column degree), ...), low, top)
#   low:   the last two rows are kept out of the generator and get degree 1 and 2
#   top:   row 0 is filled up to this degree afterwards (one row past the others: at the class's cap, or
#          past a bound); 0 leaves it alone
CODES = {
    "dc8_cpt2_rpt1": (126, 64, ((126, 3),), False, 8),                 # rows 5..6, one of 8: the cap
    "dc8_cpt4_rpt1": (252, 64, ((252, 2),), False, 0),                 # rows 7..8: the cap
    "dc8_cpt4_rpt2": (1037, 520, ((700, 3), (337, 2)), True, 8),       # rows 5..6, one of 8, and 1, 2
    "dc16_cpt2_rpt1": (126, 64, ((95, 5), (31, 3)), False, 0),         # rows 8..9: the least degree of DC 16
    "dc16_cpt4_rpt1": (252, 64, ((244, 4), (8, 6)), False, 0),         # every row 16: the cap
    "dc16_cpt4_rpt2": (1037, 520, ((900, 6), (137, 3)), True, 16),      # rows 11..12, one of 16, and 1, 2
    "dc32_cpt2_rpt1": (126, 64, ((100, 9), (26, 6)), False, 0),        # rows 16..17: the least degree of DC 32
    "dc32_cpt4_rpt1": (252, 64, ((244, 8), (8, 12)), False, 0),        # every row 32: the cap
    "dc32_cpt4_rpt2": (1037, 520, ((1000, 12), (37, 4)), True, 0),     # rows 23..24 and 1, 2
    "row26": (252, 64, ((152, 7), (100, 6)), False, 0),                # every row 26: the packed state's last
    "row27": (252, 64, ((152, 7), (100, 6)), False, 27),                # one row of 27: no flood / layered schedule
    "row33": (252, 64, ((244, 8), (8, 12)), False, 33),                 # one row of 33: no row schedule, no BP
}
# name -> (least, greatest row degree above the two low rows, DC, CPT, RPT, threads); DC None: no row schedule
SHAPES = {
    "dc8_cpt2_rpt1": (5, 8, 8, 2, 1, 64), "dc8_cpt4_rpt1": (7, 8, 8, 4, 1, 64), "dc8_cpt4_rpt2": (5, 8, 8, 4, 2, 320),
    "dc16_cpt2_rpt1": (8, 9, 16, 2, 1, 64), "dc16_cpt4_rpt1": (16, 16, 16, 4, 1, 64),
    "dc16_cpt4_rpt2": (11, 16, 16, 4, 2, 320),
    "dc32_cpt2_rpt1": (16, 17, 32, 2, 1, 64), "dc32_cpt4_rpt1": (32, 32, 32, 4, 1, 64),
    "dc32_cpt4_rpt2": (23, 24, 32, 4, 2, 320),
    "row26": (26, 26, 32, 4, 1, 64), "row27": (26, 27, 32, 4, 1, 64), "row33": (32, 33, None, 0, 0, 0),
}
ROW_CODES = [n for n in CODES if n.startswith("dc")]
MATRIX_CODES = list(CODES)
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
VARIANTS = {k: PARITY_VARIANTS[k] for k in ("ms", "nms", "oms", "qnms")}
TS = (0, 1, 3, 10)
FRAMES, SIGMA = 16, 0.7
FAMILY_SIGMA = 0.5   # BP, DD-BMP: at 0.7 the wide check nodes send next to nothing and no decision moves after T = 1
UNSUPPORTED = -4


def build_code(path, name):
    """test_frame_tail._code with a column degree per bit: each bit takes its d least loaded
    rows, ties broken by a seeded rng, so the row degrees differ by at most one and no row
    repeats within a bit."""
    N, M, degs, low, top = CODES[name]
    rng = np.random.default_rng(sorted(CODES).index(name) + 100)
    dv = np.concatenate([np.full(n, d) for n, d in degs])
    assert len(dv) == N
    free = M - 2 if low else M
    load = np.zeros(free, dtype=np.int64)
    rows = [[] for _ in range(M)]
    for i in range(N):
        for j in np.lexsort((rng.random(free), load))[:dv[i]]:
            rows[j].append(i)
            load[j] += 1
    if low:   # among the bits of the lowest column degree
        rows[M - 2], rows[M - 1] = [N - 3], [N - 2, N - 1]
    rows[0] += [i for i in range(N) if i not in rows[0]][:max(0, top - len(rows[0]))]
    H = codes.ParityCheck.from_rows(N, rows)
    codes.write_alist(H, path)
    return H


class Lab:
    """One code: its alist, the oracle, one device context, the noise frames, and every
    oracle result computed once."""

    def __init__(self, root, name):
        self.name = name
        self.path = str(root / f"{name}.alist")
        self.H = build_code(self.path, name)
        self.N, self.M = self.H.N, self.H.M
        self.deg = sorted(len(r) for r in self.H.rows)
        self.A = O.Alist(self.path)
        self.graph = native.Graph.from_alist(self.path)
        self.ctx = native.Context(self.graph, 0, 64)
        rng = np.random.default_rng(1000 + self.N + self.deg[-1])
        y = 1.0 + SIGMA * rng.standard_normal((FRAMES, self.N))
        self.y = {"f64": y, "f32": y.astype(np.float32)}
        yw = 1.0 + FAMILY_SIGMA * rng.standard_normal((FRAMES, self.N))
        self.yw = {"f64": yw, "f32": yw.astype(np.float32)}
        self.flood = functools.lru_cache(maxsize=None)(self._flood)
        self.layered = functools.lru_cache(maxsize=None)(self._layered)

    def front(self, prec, vname):
        return _oracle_front(self.y[prec], VARIANTS[vname], prec == "f32")

    def _flood(self, prec, vname, T):
        v = VARIANTS[vname]
        return self.A.decode(self.front(prec, vname), T, O.Cfg(**v))

    def _layered(self, prec, vname, T):
        order, _ = self.graph.layers()
        return self.A.decode_layered(self.y[prec], T, O.Cfg(**VARIANTS[vname]), order)

    def syndrome_fail(self, d):
        return [int(any(self.H.syndrome(row != 1))) for row in d]

    def options(self, opts):
        self.ctx.reset_options()
        self.ctx.set_options(opts)
        return self.ctx


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    assert native.device_count() > 0, "no HIP device visible"
    root = tmp_path_factory.mktemp("shapes")
    return functools.lru_cache(maxsize=None)(lambda name: Lab(root, name))


def cfg_of(prec, vname, T, **kw):
    return native.DecoderConfig(T=T, precision=PREC[prec][0], **VARIANTS[vname], **kw)


def assert_accounting(L, d, fr, cnt, want, T):
    """test_gpu_parity.test_decisions_bit_exact_vs_oracle's assertions (all-zero codeword)."""
    mism = (d != want).sum(axis=1)
    assert int(mism.sum()) == 0, f"frames {np.nonzero(mism)[0].tolist()} differ in {mism[mism > 0].tolist()} decisions"
    w = (want != 1).sum(axis=1)
    assert np.array_equal(fr["bit_err"], w)
    sf = L.syndrome_fail(want)
    assert list(fr["syndrome_fail"]) == sf
    assert cnt.frames == len(want) and cnt.bit_err == int(w.sum()) and cnt.frame_err == int((w > 0).sum())
    assert cnt.iters == T * len(want) and cnt.syndrome_fail == sum(sf)


def row_shape(ctx, cfg):
    i = ctx.row_sched_info(cfg)
    return (i["dc"], i["slots_per_thread"], i["rows_per_thread"], i["threads"]), i["cw_per_block"]


# ------------------------------------------------------------------ the codes
@pytest.mark.parametrize("name", MATRIX_CODES)
def test_codes_are_the_ones_meant(lab, name):
    """Row degrees of each code, and the discriminating input: the oracle's decisions differ
    from the channel's hard decisions and still change between T = 3 and T = 10."""
    L = lab(name)
    N, M, degs, low, top = CODES[name]
    lo, hi = SHAPES[name][:2]
    assert (L.N, L.M) == (N, M) and all(len(set(r)) == len(r) for r in L.H.rows)
    deg = L.deg[2:] if low else L.deg
    assert (deg[0], deg[-1]) == (lo, hi), (deg[0], deg[-1])
    assert not low or L.deg[:2] == [1, 2]
    assert not top or (hi == top and deg.count(hi) == 1)
    hard = np.where(L.y["f64"] > 0, 1, -1)
    assert (hard != 1).any()
    d3, d10 = L.flood("f64", "ms", 3), L.flood("f64", "ms", 10)
    assert (d3 != hard).any() and (d10 != d3).any()


def test_classes_have_their_edges():
    """Per DC class: a row at the cap, a widest row at the least degree selecting the class, a
    code with the degree-1 and degree-2 rows, and N off the multiples of 4."""
    for dc, least in ((8, None), (16, 9), (32, 17)):
        names = [n for n in ROW_CODES if SHAPES[n][2] == dc]
        assert {SHAPES[n][3:5] for n in names} == {(2, 1), (4, 1), (4, 2)}
        assert any(SHAPES[n][1] == dc for n in names)
        assert least is None or any(SHAPES[n][1] == least for n in names)
        assert any(CODES[n][3] for n in names)
        assert any(CODES[n][0] % 4 for n in names) and all(CODES[n][0] % 64 for n in names)


# ------------------------------------------------------------------ min-sum, given channel
def selections(name, prec, vname):
    """(options, kernel expected, row shape expected or None, codewords per block) of every
    kernel selection of one code: plan_rows / plan_fast_path / plan_flood as read."""
    lo, hi, dc, cpt, rpt, threads = SHAPES[name]
    shape = (dc, cpt, rpt, threads)
    out = []
    if prec == "f64":
        if dc:
            out.append((dict(), "rows_fast" if dc <= 16 else "rows", shape, 1))
            out.append((dict(rows64="rows"), "rows", shape, 1))
    elif dc:
        out.append((dict(), "rows", shape, 2 if dc == 8 else 1))
        if dc == 8:   # the pair instance: MS and NMS with the verified reciprocal; OMS keeps the row kernel
            out.append((dict(rows32="fast"), "rows" if vname == "oms" else "rows_fast", shape, 2))
    if not dc:
        out.append((dict(), "lds", None, 0))
    flood = "flood" if hi <= 26 else "global"   # no flood schedule past the packed row state: the generic kernel
    out += [(dict(kernel="lds"), "lds", None, 0), (dict(kernel="flood"), flood, None, 0),
            (dict(kernel="flood", flood_mode="persistent"), flood, None, 0), (dict(kernel="global"), "global", None, 0)]
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", MATRIX_CODES)
def test_minsum_matrix(lab, name, prec):
    """Every kernel selection x {ms, nms, oms, qnms} x T in {0, 1, 3, 10} on 16 noise frames:
    the kernel and the row shape asserted, decisions, per-frame results and counters equal
    to the flooding oracle's."""
    L = lab(name)
    ran = set()
    for vname in VARIANTS:
        for opts, kernel, shape, cpb in selections(name, prec, vname):
            ctx = L.options(opts)
            for T in TS:
                cfg = cfg_of(prec, vname, T)
                tag = (opts, vname, T)
                assert ctx.kernel_info(cfg)["kernel"] == kernel, (tag, ctx.kernel_info(cfg))
                if shape:
                    assert row_shape(ctx, cfg) == (shape, cpb), (tag, ctx.row_sched_info(cfg))
                else:
                    with pytest.raises(native.LdpcError) as e:
                        ctx.row_sched_info(cfg)
                    assert e.value.code == UNSUPPORTED
                d, fr, cnt = ctx.decode(L.y[prec], cfg)
                assert_accounting(L, d, fr, cnt, L.flood(prec, vname, T), T)
            ran.add(kernel)
    L.ctx.reset_options()
    dc = SHAPES[name][2]
    want = {"lds", "global"} | ({"flood"} if SHAPES[name][1] <= 26 else set()) | ({"rows"} if dc else set())
    if dc and (dc <= 16 if prec == "f64" else dc == 8):
        want.add("rows_fast")
    assert ran == want


def test_every_row_kernel_shape_is_reached():
    """The matrix's selections name all nine k_decode_rows shapes in both precisions, the six
    fp64 and three fp32 k_rows_fast shapes, and the flood kernels of DC 8, 16 and 32."""
    rows = {p: set() for p in PREC}
    fast = {p: set() for p in PREC}
    flood = set()
    for name in ROW_CODES:
        for prec in PREC:
            for vname in VARIANTS:
                for opts, kernel, shape, cpb in selections(name, prec, vname):
                    if kernel == "rows":
                        rows[prec].add(shape[:3])
                    if kernel == "rows_fast":
                        fast[prec].add(shape[:3])
                    if kernel == "flood":
                        flood.add(SHAPES[name][2])
    nine = {(dc, cpt, rpt) for dc in (8, 16, 32) for cpt, rpt in ((2, 1), (4, 1), (4, 2))}
    assert rows["f64"] == rows["f32"] == nine
    assert fast["f64"] == {s for s in nine if s[0] <= 16} and fast["f32"] == {s for s in nine if s[0] == 8}
    assert flood == {8, 16, 32}


def _premise_frames(N):
    """The frames of test_rows_fast.test_premise_breaks_are_redecoded_exactly."""
    y = 1.0 + SIGMA * np.random.default_rng(4242).standard_normal((16, N))
    y[1] *= 1e305                     # input premise: |yq| >= 2^1000
    y[2] *= 1e-305                    # minima far below 2^-960 (NMS fast division premise)
    y[3, 5] = np.inf                  # non-finite input
    y[4, 7] = np.nan
    y[5] *= 2.0 ** 995                # grows past 2^1000 after a few iterations
    y[6, ::3] = -0.0                  # signed zeros: canonicalised, never a premise break
    y[7] = np.where(np.arange(N) % 2 == 0, 0.5, -1.0)   # ties in every row
    return y


@pytest.mark.parametrize("vname", ["ms", "nms", "oms"])
@pytest.mark.parametrize("name", [n for n in ROW_CODES if SHAPES[n][2] <= 16])
def test_premise_breaks_are_redecoded_exactly(lab, name, vname):
    """The six fp64 k_rows_fast shapes: frames that break the fast premise are re-decoded on
    the exact path (at least frames 1, 3 and 4) and every frame equals the fp64 oracle."""
    L = lab(name)
    ctx = L.options({})
    y = _premise_frames(L.N)
    v = VARIANTS[vname]
    for T in (1, 7, 30):
        cfg = cfg_of("f64", vname, T)
        assert ctx.kernel_info(cfg)["kernel"] == "rows_fast"
        assert row_shape(ctx, cfg) == (SHAPES[name][2:], 1)
        d, fr, cnt = ctx.decode(y, cfg)
        redo = ctx.redo_count()
        want = L.A.decode(y, T, O.Cfg(**v))
        mism = (d != want).sum(axis=1)
        assert int(mism.sum()) == 0, f"T={T}: mismatching frames {np.nonzero(mism)[0].tolist()}"
        w = (want != 1).sum(axis=1)
        assert np.array_equal(fr["bit_err"], w)
        assert cnt.frames == len(y) and cnt.bit_err == int(w.sum()) and cnt.iters == T * len(y)
        assert 3 <= redo <= len(y), redo


# ------------------------------------------------------------------ min-sum, on-device channel
SEED, STREAM, FIRST_CW, EBN0, RATE = 0xC0FFEE123, 0x1234, 7, 1.0, 0.5


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ROW_CODES)
def test_on_device_channel(lab, name, prec):
    """sim_trace against the oracle on the y it returns, and sim_batch with the same seed,
    stream and first_cw against sim_trace, at batches 32 and 33 (fp32 DC = 8: the last pair
    lacks its partner), for the default kernel and the row kernel (rows_fast and rows in
    fp64; rows, and rows_fast at DC = 8, in fp32).

    sim_trace asks for the samples, so its channel step is the general loop; sim_batch asks
    for none and, with no codeword table and no front end, takes the straight-line channel
    step of k_decode_rows / k_rows_fast -- where N is a multiple of 4, which is why the
    (DC, 4, 1) codes have N = 252. At N = 126 and N = 1037 both calls take the general loop
    and sim_batch differs from sim_trace in the missing y_out and d_out only."""
    L = lab(name)
    shape = SHAPES[name][2:]
    for vname in ("ms", "nms"):
        kernels = set()
        for opts, kernel, _, cpb in selections(name, prec, vname):
            if not kernel.startswith("rows"):
                continue
            ctx = L.options(opts)
            cfg = cfg_of(prec, vname, 10)
            assert ctx.kernel_info(cfg)["kernel"] == kernel and row_shape(ctx, cfg) == (shape, cpb)
            kernels.add(kernel)
            for batch in (32, 33):
                y, d, fr, cnt = ctx.sim_trace(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, batch)
                assert y.shape == (batch, L.N) and np.isfinite(y).all()
                want = L.A.decode(y, 10, O.Cfg(**VARIANTS[vname]))
                assert_accounting(L, d, fr, cnt, want, 10)
                assert np.array_equal(fr["uncoded_bit_err"], (y <= 0).sum(axis=1))
                fr2, cnt2 = ctx.sim_batch(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, batch)
                assert np.array_equal(fr2, fr), (opts, vname, batch)
                assert np.array_equal(cnt2.as_array(), cnt.as_array()), (opts, vname, batch)
                assert cnt.bit_err > 0
        assert "rows" in kernels
    L.ctx.reset_options()


# ------------------------------------------------------------------ layered
LAYERED_CODES = ["dc8_cpt4_rpt1", "dc16_cpt4_rpt1", "dc16_cpt4_rpt2", "dc32_cpt2_rpt1", "dc32_cpt4_rpt2", "row26"]
LAYERED_DC = {"dc8_cpt4_rpt1": 8, "dc16_cpt4_rpt1": 16, "dc16_cpt4_rpt2": 16, "dc32_cpt2_rpt1": 26,
              "dc32_cpt4_rpt2": 26, "row26": 26}   # the layered_fn<., DC> instantiation of each


@pytest.mark.parametrize("name", LAYERED_CODES)
def test_layer_partition(lab, name):
    """The properties of test_layered.test_layer_partition_is_bit_disjoint. The generator
    spreads neighbouring bits over different rows, so even the rows of degree 26 in 252 bits
    leave disjoint pairs: every code here has layers of several rows (33 layers of 64 rows at
    row degree 26), which is the parallel layer update the kernels have to get right."""
    L = lab(name)
    order, ptr = L.graph.layers()
    assert sorted(order.tolist()) == list(range(L.M))
    assert ptr[0] == 0 and ptr[-1] == L.M and np.all(np.diff(ptr) > 0)
    layer_bits = []
    for k in range(len(ptr) - 1):
        cols = [c for j in order[ptr[k]:ptr[k + 1]] for c in L.H.rows[j]]
        assert len(cols) == len(set(cols)), f"layer {k} rows share a bit"
        layer_bits.append(set(cols))
    for k in range(1, len(ptr) - 1):
        assert all(layer_bits[k] & layer_bits[j] for j in range(k))
    meet = all(set(a) & set(b) for i, a in enumerate(L.H.rows) for b in L.H.rows[:i])
    assert meet == (len(ptr) - 1 == L.M)      # single-row layers exactly when no two rows are disjoint
    assert 1 < len(ptr) - 1 < L.M and int(np.diff(ptr).max()) > 1
    fsdc = SHAPES[name][1]
    assert LAYERED_DC[name] == (8 if fsdc <= 8 else 16 if fsdc <= 16 else 26)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", LAYERED_CODES)
def test_layered_matrix(lab, name, prec):
    """layered_lds and layered_global x {ms, nms, oms} x T in {0, 1, 3, 10} against
    decode_layered over Graph.layers()'s order."""
    L = lab(name)
    for opts, kernel in ((dict(), "layered_lds"), (dict(kernel="global"), "layered_global")):
        ctx = L.options(opts)
        for vname in ("ms", "nms", "oms"):
            for T in TS:
                cfg = cfg_of(prec, vname, T, schedule=native.LAYERED)
                assert ctx.kernel_info(cfg)["kernel"] == kernel
                d, fr, cnt = ctx.decode(L.y[prec], cfg)
                assert_accounting(L, d, fr, cnt, L.layered(prec, vname, T), T)
    L.ctx.reset_options()
    assert (L.layered(prec, "ms", 10) != L.flood(prec, "ms", 10)).any()   # another schedule, another result


# ------------------------------------------------------------------ the 26 / 27 and 32 / 33 bounds
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_packed_state_bound(lab, prec):
    """Row degree 26 has the flood and the layered schedule (both exact: the matrix tests);
    one row of 27 has neither: a layered config is refused, kernel = flood falls to the
    generic global kernel and the default stays the DC = 32 row kernel, all exact."""
    cfg = cfg_of(prec, "nms", 3)
    lay = cfg_of(prec, "nms", 3, schedule=native.LAYERED)
    L26, L27 = lab("row26"), lab("row27")
    assert L26.deg[-1] == 26 and L27.deg[-2:] == [26, 27]
    assert L26.options(dict(kernel="flood")).kernel_info(cfg)["kernel"] == "flood"
    assert L26.options({}).kernel_info(lay)["kernel"] == "layered_lds"
    ctx = L27.options({})
    for call in (lambda: ctx.kernel_info(lay), lambda: ctx.decode(L27.y[prec], lay)):
        with pytest.raises(native.LdpcError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    for opts, kernel in ((dict(), "rows"), (dict(kernel="flood"), "global"),
                         (dict(kernel="flood", flood_mode="persistent"), "global")):
        ctx = L27.options(opts)
        assert ctx.kernel_info(cfg)["kernel"] == kernel
        d, fr, cnt = ctx.decode(L27.y[prec], cfg)
        assert_accounting(L27, d, fr, cnt, L27.flood(prec, "nms", 3), 3)
    L27.ctx.reset_options()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_row_schedule_and_bp_bound(lab, prec):
    """Row degree 32 has the row schedule and BP (exact: the matrix and BP tests); one row of 33
    has no row schedule -- the default is the generic LDS kernel -- flooding min-sum stays
    exact on lds and global, and BP is refused."""
    cfg = cfg_of(prec, "nms", 3)
    bp = native.DecoderConfig(variant=native.BP, T=3, precision=PREC[prec][0], n0=1.0)
    L32, L33 = lab("dc32_cpt4_rpt1"), lab("row33")
    assert L32.deg[-1] == 32 and L33.deg[-2:] == [32, 33]
    assert row_shape(L32.options({}), cfg)[0] == (32, 4, 1, 64)
    assert L32.ctx.kernel_info(bp)["kernel"] == "bp_lds"
    ctx = L33.options({})
    for call in (lambda: ctx.row_sched_info(cfg), lambda: ctx.kernel_info(bp), lambda: ctx.decode(L33.y[prec], bp)):
        with pytest.raises(native.LdpcError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    for opts, kernel in ((dict(), "lds"), (dict(kernel="lds"), "lds"), (dict(kernel="global"), "global")):
        ctx = L33.options(opts)
        assert ctx.kernel_info(cfg)["kernel"] == kernel
        d, fr, cnt = ctx.decode(L33.y[prec], cfg)
        assert_accounting(L33, d, fr, cnt, L33.flood(prec, "nms", 3), 3)
    L33.ctx.reset_options()


# ------------------------------------------------------------------ the other decoder families
WIDE = ["dc16_cpt4_rpt1", "dc32_cpt4_rpt1"]   # M = 64, every row 16 / every row 32
N0 = 2.0 * FAMILY_SIGMA * FAMILY_SIGMA          # the noise of Lab.yw


@pytest.mark.parametrize("name", WIDE)
def test_bp_f64_equals_oracle(lab, name):
    """k_bp_lds<., 16> and k_bp_lds<., kBpMaxDc> (the row-32 code is accepted): exact."""
    L = lab(name)
    ctx = L.options({})
    y = L.yw["f64"]
    yq = np.array([L.A.bp_front(row, N0) for row in y])
    for T in (0, 1, 4, 20):
        cfg = native.DecoderConfig(variant=native.BP, T=T, precision=native.F64, n0=N0)
        assert ctx.kernel_info(cfg)["kernel"] == "bp_lds"
        d, fr, cnt = ctx.decode(y, cfg)
        want = L.A.bp_decode(yq, T)
        assert int((d != want).sum()) == 0, f"T={T}"
        w = (want != 1).sum(axis=1)
        assert np.array_equal(fr["bit_err"], w) and cnt.bit_err == int(w.sum()) and cnt.iters == T * len(y)
        assert np.array_equal(fr["uncoded_bit_err"], (yq < 0).sum(axis=1))
    assert (L.A.bp_decode(yq, 4) != L.A.bp_decode(yq, 1)).any()   # decisions still move after the first iteration
    ctx.set_option("kernel", "global")   # the min-sum option does not move BP
    assert ctx.kernel_info(cfg)["kernel"] == "bp_lds"
    L.ctx.reset_options()


@pytest.mark.parametrize("name", WIDE)
def test_bp_f32_within_tolerance(lab, name):
    """test_bp.test_bp_f32_decisions_within_tolerance on the wide rows: at most F32_BIT_TOL of
    the decisions differ from the fp32 oracle, and a frame the oracle decodes must decode."""
    L = lab(name)
    ctx = L.options({})
    y = L.yw["f32"]
    yq = np.clip((np.float32(4) * y) / np.float32(N0), -20, 20).astype(np.float32)
    for T in (0, 1, 4, 20):
        cfg = native.DecoderConfig(variant=native.BP, T=T, precision=native.F32, n0=N0)
        assert ctx.kernel_info(cfg)["kernel"] == "bp_lds"
        d, fr, _ = ctx.decode(y, cfg)
        want = L.A.bp_decode(yq, T)
        assert (d != want).mean() <= F32_BIT_TOL, f"T={T}: {(d != want).sum()} decisions differ"
        ok = (want == 1).all(axis=1)
        assert (fr["bit_err"][ok] == 0).all(), f"T={T}: a frame the oracle decodes failed on the GPU"


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("vname", ["SMNGDBF", "MGDBF"])
@pytest.mark.parametrize("name", WIDE)
def test_gdbf_equals_oracle(lab, name, vname, prec):
    """test_gdbf.test_gdbf_decisions_bit_exact_vs_oracle on the generic kernel (gdbf_lds)."""
    from test_gdbf import COMMON, GPU_VARIANTS, _gpu_cfg
    L = lab(name)
    ctx = L.options({})
    c = dict(COMMON, **GPU_VARIANTS[vname])
    cfg = O.GdbfCfg(**c)
    dt = PREC[prec][1]
    g = O.GlibcRandom(77 + len(vname))
    B, sigma = 6, 0.5
    y = np.stack([g.channel(np.ones(L.N, dtype=np.int32), sigma) for _ in range(B)]).astype(dt)
    pert = g.rann_fill(B * cfg.T * L.N, sigma * cfg.noise_scale).reshape(B, cfg.T, L.N).astype(dt)
    use_pert = cfg.flags & O.GDBF_NOISE
    gcfg = _gpu_cfg(native, c, prec == "f32")
    assert ctx.gdbf_kernel_info(gcfg)["kernel"] == "gdbf_lds"
    d, fr, cnt = ctx.gdbf_decode(y, pert if use_pert else None, gcfg)
    its = []
    for b in range(B):
        want, it, sat = L.A.gdbf_decode(y[b], pert[b] if use_pert else None, cfg)
        assert int((d[b] != want).sum()) == 0, b
        assert fr["iters"][b] == it and fr["bit_err"][b] == int((want != 1).sum())
        its.append(it)
    assert cnt.iters == sum(its) and cnt.frames == B
    assert max(its) > 0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", WIDE)
def test_ddbmp_equals_restatement(lab, name, prec):
    from test_ddbmp import FRONT, same
    from test_ddbmp import cfg_of as ddbmp_cfg
    L = lab(name)
    ctx = L.options({})
    o = D.Ddbmp(L.path)
    y = L.yw[prec]
    for T in (0, 1, 2, 30):
        cfg = ddbmp_cfg(prec, T)
        assert ctx.kernel_info(cfg)["kernel"] == "ddbmp_lds"
        rd, rfr = o.decode(y, T, dtype=PREC[prec][1], **FRONT)
        d, fr, cnt = ctx.decode(y, cfg)
        assert np.array_equal(d, rd), T
        same(fr, rfr)
        assert cnt.as_dict()["iters"] == int(rfr["iters"].sum())
    assert 0 < (rfr["iters"] < 30).sum() < len(y)   # early stops and frames that never stop


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", WIDE)
def test_rgdbf_equals_restatement(lab, name, prec):
    from test_rgdbf import cfg_of as rgdbf_cfg
    L = lab(name)
    ctx = L.options({})
    o = RO.Rgdbf(L.path)
    T, maxphase = 20, 3
    y, pert = RO.glibc_frames(o, 0.5, 6.0, 0.75, maxphase * T, 3, 6)   # sigma 0.5
    cfg = rgdbf_cfg(prec, alpha=1.2, T=T, maxphase=maxphase)
    assert ctx.rgdbf_kernel_info(cfg)["kernel"] == "rgdbf_lds"
    rd, rfr = o.decode(y, pert, T=T, maxphase=maxphase, flags=native.RGDBF_FLAGS, alpha=1.2, dtype=PREC[prec][1])
    d, fr, cnt = ctx.rgdbf_decode(y, pert, cfg)
    assert np.array_equal(fr["iters"], rfr["iters"]), (fr["iters"], rfr["iters"])
    assert np.array_equal(d, rd)
    for k in ("bit_err", "uncoded_bit_err", "syndrome_fail"):
        assert np.array_equal(np.asarray(fr[k], dtype=np.int64), rfr[k]), k
    assert cnt.as_dict()["iters"] == int(rfr["iters"].sum())
    assert 0 < (rfr["iters"] < maxphase * T).sum() < len(y)   # a frame that stops and frames that exhaust the phases
