"""include/sts_cross.h on the device: sts_cross_moments (csrc/sts_cross.hip) against exact arithmetic,
at every seam of its kernels, beside poisoned series, bit for bit where the header promises bits, in
awkward layouts, behind a delayed stream and through the `_host` twin.

Bar (the issue's): |got - exact| <= 1e-10 sqrt(C_ii C_jj) / (T - 1) for COV, 1e-10 absolute for CORR;
cross_ref.errors gives the error in those units.  The families are held to cross_ref.exact (60
digits); the seam shapes, which 60-digit arithmetic is too slow for, to the numpy restatement, which
sits within 3e-15 of exact() on every family (tests/test_cross_cpu.py).  Means: within T 2^-53 of
the series' largest magnitude, the bound of any summation order.

Seams.  The kernel's sizes are read from the header (STS_CROSS_TILE / _CHUNK / _SPLIT); the tile count
below which a long T is split over workgroups is STS_CROSS_SPLIT_TILES of csrc/sts_cross.hip, written
once here.  S in {1, 15, 16, 17} and either side of the tile; T in {2, 3, 4, 5}, either side of the
LDS stage and of the split (one workgroup per segment and a finalise kernel, as S = 17 always is),
and test_split_and_walked_plans_agree takes the smallest panel whose tiles fill the chip, so one
workgroup walks two segments, and finds the split plan's bits in its corners.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cross_ref as cr
import layout_arena as la
import stream_gate as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sts_cross.h")).read()
TILE, CHUNK, SPLIT = (int(re.search(r"#define STS_CROSS_%s (\d+)" % n, HEADER).group(1)) for n in ("TILE", "CHUNK", "SPLIT"))
SPLIT_TILES = 512          # -DSTS_CROSS_SPLIT_TILES
KINDS = ("cov", "corr")
POISON_OUT = -3.0e55
T_SMALL = 2 * CHUNK + 5    # odd, three LDS stages, the last one partial


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def delay(torch):
    return sg.calibrate(torch)[0]


def lib():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def hv(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def dev(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device="cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Out:
    pass


def run(torch, x, y=None, kind="cov", means=True, host=False):
    """one call on packed panels -> Out(out, mx, my) as numpy; x / y numpy or device tensors"""
    code = KINDS.index(kind)
    L, o = lib(), Out()
    Sx, T = x.shape
    Sy = 0 if y is None else y.shape[0]
    cols = Sx if y is None else Sy
    if host:
        x = np.ascontiguousarray(x)
        y = None if y is None else np.ascontiguousarray(y)
        o.out = np.full((Sx, cols), POISON_OUT)
        o.mx = np.full(Sx, POISON_OUT) if means else None
        o.my = np.full(cols, POISON_OUT) if means and y is not None else None
        st = L.sts_cross_moments_host(hv(x), Sx, T, T, hv(y), Sy, T, code, hv(o.out), hv(o.mx), hv(o.my))
        assert st == 0, L.sts_last_error()
        return o
    dx = x if hasattr(x, "data_ptr") else dev(torch, x)
    dy = None if y is None else (y if hasattr(y, "data_ptr") else dev(torch, y))
    full = lambda *shape: torch.full(shape, POISON_OUT, dtype=torch.float64, device="cuda:0")
    out = full(Sx, cols)
    mx = full(Sx) if means else None
    my = full(cols) if means and y is not None else None
    st = L.sts_cross_moments(vp(dx), Sx, T, T, vp(dy), Sy, T, code, vp(out), cols, vp(mx), vp(my), None)
    assert st == 0, L.sts_last_error()
    torch.cuda.synchronize()
    get = lambda t: None if t is None else t.cpu().numpy()
    o.out, o.mx, o.my = get(out), get(mx), get(my)
    return o


def check(o, ref, kind, x, y=None, what=""):
    e = cr.errors(o.out, ref, kind)
    em = cr.mean_error(o.mx, ref["mean_x"], x)
    print(what, kind, "error / bar's unit %.3g, mean %.3g" % (e, em))
    assert e <= cr.BAR, (what, kind, e)
    assert em <= cr.mean_bar(x.shape[1]), (what, em)
    if y is not None:
        assert cr.mean_error(o.my, ref["mean_y"], y) <= cr.mean_bar(x.shape[1])


def noise(seed, S, T):
    return np.random.default_rng([77, seed, S, T]).standard_normal((S, T))


# ---------------- the numeric bar on the families ----------------

@functools.lru_cache(maxsize=None)
def family_case(name):
    x = cr.family(name, cr.HARD_T)
    y = cr.family(name, cr.HARD_T, seed=1)[:3]
    return x, y, cr.exact(x), cr.exact(x, y)


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_families_against_exact_arithmetic(torch, name):
    x, y, ex_sym, ex_cross = family_case(name)
    for kind in KINDS:
        check(run(torch, x, None, kind), ex_sym, kind, x, what=name + " sym")
        check(run(torch, x, y, kind), ex_cross, kind, x, y, what=name + " cross")
    c = run(torch, x, None, "corr").out
    assert c.min() <= -1.0 + 1e-6 and c.min() >= -1.0 and (np.diag(c) == 1.0).all()


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_golden_cases(torch, name):
    g = cr.load_golden()[name]
    x, y = cr.golden_case(name)
    assert [x[0, 0], x[-1, -1], y[-1, -1]] == g["probe"], "the case is not the fixture's"
    for kind in KINDS:
        check(run(torch, x, None, kind), g["sym"], kind, x, what=name + " golden sym")
        check(run(torch, x, y, kind), g["cross"], kind, x, y, what=name + " golden cross")


# ---------------- seams ----------------

S_SEAMS = sorted({1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 2})
S_TOP = 2 * TILE + 2


@functools.lru_cache(maxsize=None)
def s_panel():
    x = noise(1, S_TOP, T_SMALL)
    x[3] = -x[0]
    return x, cr.restated(x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", S_SEAMS)
def test_series_count_seams_and_the_corner_bit_for_bit(torch, S, kind):
    """every S against the restatement; and the first S rows of the 2 tile + 2 panel give that panel's
    S x S corner bit for bit (the first 17 rows of a 130-series panel, and every other seam)"""
    x, ref = s_panel()
    top = run(torch, x, None, kind)
    check(top, ref, kind, x, what="S=%d" % S_TOP)
    o = run(torch, x[:S], None, kind)
    assert same(o.out, top.out[:S, :S]) and same(o.mx, top.mx[:S])
    assert same(o.out, o.out.T)


CROSS_SHAPES = [(17, 1), (17, 8), (TILE + 1, 8), (1, S_TOP), (S_TOP, TILE + 1), (TILE, TILE), (8, 17)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Sx,Sy", CROSS_SHAPES)
def test_cross_form_shapes(torch, Sx, Sy, kind):
    """Sx != Sy against the restatement, and bit for bit the off-diagonal block of the symmetric
    matrix of the two panels stacked: an entry depends on its two rows, not on which form computed it"""
    x, y = noise(2, Sx, T_SMALL), noise(3, Sy, T_SMALL)
    o = run(torch, x, y, kind)
    check(o, cr.restated(x, y), kind, x, y, what="%dx%d" % (Sx, Sy))
    both = run(torch, np.vstack([x, y]), None, kind)
    assert same(o.out, both.out[:Sx, Sx:]) and same(o.mx, both.mx[:Sx]) and same(o.my, both.mx[Sx:])
    back = run(torch, y, x, kind)
    assert same(back.out, o.out.T)


T_SEAMS = sorted({2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT + 3})


@pytest.mark.parametrize("T", T_SEAMS)
def test_length_seams(torch, T):
    x, y = noise(4, 17, T), noise(5, 8, T)
    x[5] = -x[2]
    ref_s, ref_c = cr.restated(x), cr.restated(x, y)
    for kind in KINDS:
        o = run(torch, x, None, kind)
        check(o, ref_s, kind, x, what="T=%d sym" % T)
        assert same(o.out, o.out.T)
        check(run(torch, x, y, kind), ref_c, kind, x, y, what="T=%d cross" % T)


def test_split_and_walked_plans_agree(torch):
    """Sums over T are closed every STS_CROSS_SPLIT steps and merged in ascending order, by one workgroup
    per segment and a finalise kernel (few tiles) or by the workgroup that walks them all (tiles that fill
    the chip).  The smallest panel of the second kind, two segments: its corners are, bit for bit, what
    17 series alone give in the first."""
    n = 1
    while n * (n + 1) // 2 < SPLIT_TILES:
        n += 1
    S, T = n * TILE, SPLIT + 1
    g = torch.Generator(device="cuda:0")
    g.manual_seed(11)
    x = torch.randn((S, T), dtype=torch.float64, device="cuda:0", generator=g)
    for kind in KINDS:
        big = run(torch, x, None, kind)
        head, tail = x[:17].contiguous(), x[S - 17:].contiguous()
        for sub, sl in ((head, slice(0, 17)), (tail, slice(S - 17, S))):
            o = run(torch, sub, None, kind)
            assert same(o.out, big.out[sl, sl]) and same(o.mx, big.mx[sl])
            xs = sub.cpu().numpy()
            check(o, cr.restated(xs), kind, xs, what="corner of S=%d" % S)
        far = run(torch, head, tail, kind)
        assert same(far.out, big.out[:17, S - 17:]) and same(far.out.T, big.out[S - 17:, :17])


# ---------------- isolation ----------------

def poison(x, row, what):
    x = x.copy()
    if what == "nan_first":
        x[row, 0] = np.nan
    elif what == "nan_last":
        x[row, -1] = np.nan
    elif what == "inf":
        x[row, x.shape[1] // 2] = -np.inf
    elif what == "constant":
        x[row] = 0.1                    # its mean does not round to itself: the rule, not the arithmetic, gives +0.0
    elif what == "zero":
        x[row] = 0.0
    return x


ISO_S = TILE + 17                       # one whole tile and a partial one
ISO_ROWS = list(range(16, 32)) + [ISO_S - 1]      # every position mod 16 of one tile; the last row of the partial tile


@functools.lru_cache(maxsize=None)
def iso_clean(kind):
    import torch
    x = noise(7, ISO_S, T_SMALL)
    return x, run(torch, x, None, kind), run(torch, x[:17], x, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("what", ["nan_first", "nan_last", "inf", "constant", "zero"])
def test_a_poisoned_series_changes_its_own_row_and_column_only(torch, what, kind):
    x, clean, clean_cross = iso_clean(kind)
    nan = what in ("nan_first", "nan_last", "inf")
    for row in ISO_ROWS:
        xp = poison(x, row, what)
        o = run(torch, xp, None, kind)
        others = np.ones(ISO_S, dtype=bool)
        others[row] = False
        blk = np.ix_(others, others)
        assert same(o.out[blk], clean.out[blk]), (what, row)
        assert same(o.mx[others], clean.mx[others])
        line = np.concatenate([o.out[row], o.out[:, row]])
        if nan:
            assert np.isnan(line).all() and np.isnan(o.mx[row])
        else:
            assert abs(o.mx[row] - xp[row, 0]) <= cr.mean_bar(T_SMALL) * abs(xp[row, 0])
            if kind == "corr":
                assert np.isnan(line).all()                                  # the diagonal included
            else:
                assert (line == 0).all() and not np.signbit(line).any()
        if kind == "corr":
            assert (np.diag(o.out)[others] == 1.0).all()
        # the cross form: the poisoned series of y owns a column
        c = run(torch, x[:17], xp, kind)
        assert same(c.out[:, others], clean_cross.out[:, others]) and same(c.mx, clean_cross.mx)
        col = c.out[:, row]
        assert np.isnan(col).all() if (nan or kind == "corr") else ((col == 0).all() and not np.signbit(col).any())


def test_two_poisons_meet(torch):
    """a NaN series against a constant one is NaN (the NaN rule comes first); constant against constant
    is +0.0 / NaN"""
    x = noise(8, 20, T_SMALL)
    x[2, 1] = np.nan
    x[18] = 3.0
    x[19] = -7.5
    cov, corr = run(torch, x, None, "cov").out, run(torch, x, None, "corr").out
    assert np.isnan(cov[2, 18]) and np.isnan(cov[18, 2]) and np.isnan(corr[2, 18])
    assert cov[18, 19] == 0 and cov[18, 18] == 0 and not np.signbit(cov[18, 18:]).any() and np.isnan(corr[18, 18:]).all()
    ref = cr.restated(x)
    for kind, got in (("cov", cov), ("corr", corr)):
        assert cr.errors(got, ref, kind) <= cr.BAR


# ---------------- reproducibility ----------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [T_SMALL, SPLIT + CHUNK + 1])
def test_bits_depend_on_the_two_rows_alone(torch, T, kind):
    S = S_TOP if T == T_SMALL else TILE + 3
    x = noise(9, S, T)
    a = run(torch, x, None, kind)
    assert same(a.out, a.out.T), "the symmetric form is exactly symmetric"
    b = run(torch, x, None, kind)
    assert same(a.out, b.out) and same(a.mx, b.mx), "two calls"
    perm = np.random.default_rng(10).permutation(S)
    p = run(torch, x[perm], None, kind)
    assert same(p.out, a.out[np.ix_(perm, perm)]) and same(p.mx, a.mx[perm]), "a row permutation permutes the bits"
    c = run(torch, x, x.copy(), kind)
    if kind == "corr":
        d = np.arange(S)
        assert np.abs(c.out[d, d] - 1.0).max() <= cr.BAR      # the cross form has no unit-diagonal rule
        c.out[d, d] = 1.0
    assert same(c.out, a.out) and same(c.my, a.mx), "y = a copy of x"
    # neighbours: the same 17 rows inside other data
    other = noise(12, S, T)
    other[20:37] = x[:17]
    q = run(torch, other, None, kind)
    assert same(q.out[20:37, 20:37], a.out[:17, :17])


# ---------------- layout ----------------

@pytest.mark.parametrize("pname", list(la.POISONS))
@pytest.mark.parametrize("lay", la.LAYOUT_NAMES)
@pytest.mark.parametrize("T", [T_SMALL, T_SMALL + 1, SPLIT + 3])
@pytest.mark.parametrize("form", ["sym", "cross"])
def test_layout(torch, form, T, lay, pname):
    """ld > T with poisoned gaps, bases that are 8-byte but not 16-byte aligned, odd and even T (the
    16-byte loads apply to an aligned base with an even ld, the last step of an odd T is loaded alone),
    ld_o > Sy with gaps that survive, red zones around every output: the packed call's bits"""
    pv = la.POISONS[pname]
    Sx, Sy = (TILE + 1, 0) if form == "sym" else (17, 8)
    x = noise(13, Sx, T)
    y = None if form == "sym" else noise(14, Sy, T)
    cols = Sx if y is None else Sy
    ld_x, ld_o_extra, bi, bo = la.layout(lay, T)
    ld_o = cols + (ld_o_extra - T)
    for kind in KINDS:
        want = run(torch, x, y, kind)
        ax = la.carve(Sx, T, ld_x, bi, pv, data=x)
        ay = None if y is None else la.carve(Sy, T, ld_x + 2, (bi + 1) % 16, pv, data=y)
        ao = la.carve(Sx, cols, ld_o, bo, la.OUT_FILL)
        amx = la.carve(1, Sx, Sx, (bo + 3) % 16, la.OUT_FILL)
        amy = None if y is None else la.carve(1, Sy, Sy, 1, la.OUT_FILL)
        ins = [a for a in (ax, ay) if a is not None]
        outs = [a for a in (ao, amx, amy) if a is not None]
        snaps_in, snaps_out = [a.snapshot() for a in ins], [a.snapshot() for a in outs]
        st = lib().sts_cross_moments(ctypes.c_void_p(ax.ptr), Sx, T, ld_x, ctypes.c_void_p(ay.ptr) if ay else None, Sy,
                                     ld_x + 2, KINDS.index(kind), ctypes.c_void_p(ao.ptr), ld_o, ctypes.c_void_p(amx.ptr),
                                     ctypes.c_void_p(amy.ptr) if amy else None, None)
        assert st == 0, lib().sts_last_error()
        torch.cuda.synchronize()
        for a, s in zip(ins, snaps_in):
            a.verify_all(s)
        for a, s in zip(outs, snaps_out):
            a.verify_outside(s)
        assert same(ao.data(), want.out) and same(amx.data()[0], want.mx)
        if amy:
            assert same(amy.data()[0], want.my)


def test_means_are_optional(torch):
    x, y = noise(15, 17, T_SMALL), noise(16, 8, T_SMALL)
    for kind in KINDS:
        assert same(run(torch, x, None, kind, means=False).out, run(torch, x, None, kind).out)
        assert same(run(torch, x, y, kind, means=False).out, run(torch, x, y, kind).out)


# ---------------- the host path ----------------

@pytest.mark.parametrize("form", ["sym", "cross"])
@pytest.mark.parametrize("S,T", [(TILE + 1, T_SMALL), (17, SPLIT + 1)])
def test_host_path_has_the_device_bits(torch, S, T, form):
    x = noise(17, S, T)
    x[1, 3] = np.nan
    x[2] = 5.0
    y = None if form == "sym" else noise(18, 8, T)
    for kind in KINDS:
        d, h = run(torch, x, y, kind), run(torch, x, y, kind, host=True)
        assert same(d.out, h.out) and same(d.mx, h.mx) and (y is None or same(d.my, h.my))
    # host rows ld apart, the pad poisoned; the means left out
    ld = T + 3
    arena = np.full((S, ld), np.nan)
    arena[:, :T] = x
    out = np.full((S, S), POISON_OUT)
    st = lib().sts_cross_moments_host(hv(arena), S, T, ld, None, 0, 0, 0, hv(out), None, None)
    assert st == 0, lib().sts_last_error()
    assert same(out, run(torch, x, None, "cov").out)


# ---------------- stream order ----------------

def _gate_case(torch, form):
    Sx, Sy, T = 17, (0 if form == "sym" else 8), SPLIT + 3         # the split plan: three kernels and the scratch
    gx = sg.GIn(torch, *[noise(s, Sx, T) for s in (20, 21, 22)])
    gy = None if form == "sym" else sg.GIn(torch, *[noise(s, Sy, T) for s in (23, 24, 25)])
    cols = Sx if gy is None else Sy
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda:0")
    out, mx, my = mk(Sx, cols), mk(Sx), (None if gy is None else mk(Sy))

    def call(st):
        return lib().sts_cross_moments(vp(gx.buf), Sx, T, T, vp(gy.buf) if gy else None, Sy, T, 1, vp(out), cols, vp(mx),
                                       vp(my), st)

    def check_(outs, host):
        x = gx.real.cpu().numpy()
        y = None if gy is None else gy.real.cpu().numpy()
        o = Out()
        o.out, o.mx, o.my = outs[0], outs[1], (outs[2] if gy else None)
        check(o, cr.restated(x, y), "corr", x, y, what="gated " + form)
    return sg.Case([g for g in (gx, gy) if g], [t for t in (out, mx, my) if t is not None], call, check_)


@pytest.mark.parametrize("form", ["sym", "cross"])
def test_gated_call_is_stream_ordered(torch, delay, form):
    """The `void* stream` entry point of sts_cross.h behind a delayed stream (tests/stream_gate.py): the
    plain call's bits, nothing written late, and the call returned while the gate was shut."""
    case = _gate_case(torch, form)
    st, res, host = sg.plain(torch, case)
    assert st == 0, lib().sts_last_error()
    case.check([r.cpu().numpy() for r in res], host)
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    pending = t.pending_at_return
    late = sg.finish(torch, t)
    assert t.status == 0
    for i, (s, r) in enumerate(zip(t.snaps, res)):
        assert sg.same_bits(s, r), "%s: output %d of the gated call differs from the plain call" % (form, i)
    assert not late, late
    assert pending, "sts_cross_moments is expected to return before its work ran"


def test_every_stream_entry_point_is_gated():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    names = sorted(m.group(1) for m in re.finditer(r"\bint\s+(sts_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                   if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip()))
    assert names == ["sts_cross_moments"]


@pytest.mark.parametrize("which", ["cov", "corr", "cov_y", "corr_y"])
def test_mirror_on_a_side_stream(torch, delay, which):
    """stats.cov / stats.corr on a non-default current stream, behind a delay: the plain call's bits, and
    the call returns while the gate is shut.  One library call per gate: the call frees its stream-ordered
    scratch on the gated stream, and the runtime makes the NEXT stream-ordered allocation on that stream
    wait on the host for the pending free -- measured for two consecutive stats.ols calls just as for two
    of these, a property of the scratch every entry point shares, not of this one."""
    from sparkts import stats
    g = sg.GIn(torch, *[noise(s, 17, 390) for s in (30, 31, 32)])
    yd = dev(torch, noise(33, 3, 390))
    fn = stats.cov if which.startswith("cov") else stats.corr
    kind = which.split("_")[0]
    run_ = (lambda x: [fn(x, yd)]) if which.endswith("_y") else (lambda x: [fn(x)])
    g.buf.copy_(g.real)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in run_(g.buf)]
    torch.cuda.synchronize()
    g.buf.copy_(g.decoy)
    torch.cuda.synchronize()
    stream, ev = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay)
        ev.record(stream)
        g.buf.copy_(g.real, non_blocking=True)
        res = run_(g.buf)
        shut_after = not ev.query()
        g.buf.copy_(g.decoy2, non_blocking=True)
        got = [t.cpu().numpy() for t in res]
    stream.synchronize()
    torch.cuda.synchronize()
    assert shut_after, "the mirror is expected to return without waiting for the device"
    for a, b in zip(got, want):
        assert same(a, b)
    x = g.real.cpu().numpy()
    y = yd.cpu().numpy() if which.endswith("_y") else None
    assert same(want[0], run(torch, x, y, kind).out)
    assert cr.errors(want[0], cr.restated(x, y), kind) <= cr.BAR
