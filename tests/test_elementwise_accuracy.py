"""The float elementwise functors of csrc/md_ops.h, tested the way the matrix products are: to the ulp against a wider
reference, to the bit against NumPy where NumPy is correctly rounded, and to the bit against THEMSELVES on every kernel that
compiles them (eager streaming / transposed / axes / generic kernels, the narrow kernels, the interpreter, the kernels hiprtc
generates at run time).

A. accuracy: sin cos tan sinh cosh tanh exp log sqrt and float power against the same NumPy function in np.longdouble, in ulps
   of the result type, over ~1.4 M stress arguments (every exponent, subnormals, infinities, NaNs, every multiple of pi/2 up to
   the cut-over of the hand-written float32 sin / cos, the overflow thresholds, random blocks).
   Bounds: float32 4 ulp (what md_ops.h quotes for NumPy's own float32 loops), float32 sin / cos 2 ulp (the recorded maxima are
   1.47 .. 1.59; the next half-ulp step), float64 4 ulp, sqrt exact. They are NOT taken from the code under test.
B. absolute negative sign ceil floor sqrt, the arithmetic / maximum / minimum / comparison functors: bit for bit NumPy, in float32,
   float64 and float16; float16 transcendentals within one float16 rounding of the float32 budget.
C. every functor gives the bits of the contiguous eager kernel on every other path.
D. chains (x*y + z ...) give the bits of the eager calls when fused: a generated kernel must not contract a*b + c into one
   rounding, because neither the eager kernels, nor the interpreter, nor NumPy do.

Twins: the unmarked tests run on the CPU double (host logic, g++'s compilation of the functors), the gpu tests on the device.
The per-function maxima are printed; the device run's table is kept as profiles/elementwise_ulp.txt."""
import ctypes as C

import numpy as np
import pytest

from minidiff_amd import ndarray as nd

gpu = pytest.mark.gpu

LD = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64      # the wider reference type
HAVE_LD = LD is np.longdouble
FUNCS = "sin cos tan sinh cosh tanh exp log sqrt".split()
UNARY_EXACT = "absolute negative sign ceil floor sqrt".split()
BINARY_EXACT = ("add subtract multiply true_divide floor_divide mod maximum minimum "
                "equal not_equal less less_equal greater greater_equal").split()
UNARY_ALL = UNARY_EXACT + FUNCS[:-1] + ["logical_not", "isnan"]
BINARY_ALL = BINARY_EXACT + ["power", "logical_and", "logical_or", "logical_xor"]
BOUND = {np.float32: 4.0, np.float64: 4.0}
BOUND_SINCOS32 = 2.0


class _Ctx:
    def __init__(self, lib, on_gpu, mdopt, capsys):
        self.lib, self.on_gpu, self.mdopt, self.capsys = lib, on_gpu, mdopt, capsys
        self.tag = "device" if on_gpu else "cpu-double"

    def say(self, line):
        with self.capsys.disabled():
            print(line)

    def jit_launched(self):
        st = (C.c_int64 * 2)()
        self.lib.vm_jit_stats(st)
        return int(st[1])


def _twin(fn):
    def cpu(lib, on_gpu, mdopt, capsys):
        if on_gpu:
            pytest.skip("other twin")
        fn(_Ctx(lib, False, mdopt, capsys))

    def dev(lib, on_gpu, mdopt, capsys):
        assert on_gpu
        fn(_Ctx(lib, True, mdopt, capsys))
    cpu.__doc__ = dev.__doc__ = fn.__doc__
    return cpu, gpu(dev)


# ---------------------------------------------------------------------------------------------------------------- arguments
_CACHE = {}


def teardown_module(module):
    """the stress sets, permutations and longdouble references (~200 MB) go back to the tests that follow"""
    _CACHE.clear()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _make_stress32():
    rng = np.random.default_rng(20240)
    inf = np.float32(np.inf)
    parts = []
    # exponent grid: zeros, subnormals, every binade, infinities, NaNs
    mant = np.concatenate([np.array([0, 1, 2, 0x400000, 0x7FFFFE, 0x7FFFFF], np.uint32), rng.integers(0, 1 << 23, 58).astype(np.uint32)])
    grid = ((np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)) | mant[None, :]).ravel()
    parts.append(np.concatenate([grid, grid | np.uint32(0x80000000)]).view(np.float32))
    # the float32 nearest to k pi/2 and its two neighbours, up to beyond the cut-over of md_sincos_small (|x| = 105615)
    c = (np.arange(1, 67300, dtype=np.float64) * (np.pi / 2)).astype(np.float32)
    nb = np.concatenate([np.nextafter(c, -inf), c, np.nextafter(c, inf)])
    parts += [nb, -nb]
    # neighbourhoods: the cut-over, the overflow / underflow thresholds of exp, sinh and cosh, tanh's saturation, ...
    up = dn = np.array([105615, 88.72283, -87.33654, -103.97, 89.41598, 9.0106, 1, 0.5, np.log(2), 2.0 ** -12, 0, 20, 1e4, 1e9,
                        np.finfo(np.float32).max], dtype=np.float32)
    acc = [up]
    with np.errstate(all="ignore"):
        for _ in range(32):
            up, dn = np.nextafter(up, inf), np.nextafter(dn, -inf)
            acc += [up, dn]
    hood = np.concatenate(acc)
    parts += [hood, -hood]
    # random blocks
    n = 160000
    parts.append(rng.standard_normal(n))
    for s in (100.0, 1e5, 1e6, 1e9):
        parts.append(rng.uniform(-s, s, n))
    parts.append(np.exp(rng.uniform(-100.0, 88.0, n)) * rng.choice([-1.0, 1.0], n))
    return np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])


def _stress(dt):
    """~1.4 M float32 stress arguments; float64: the same values widened; float16: all 65536 bit patterns."""
    if dt is np.float16:
        return _cached("s16", lambda: np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16))
    s32 = _cached("s32", _make_stress32)
    with np.errstate(all="ignore"):
        return s32 if dt is np.float32 else _cached("s64", lambda: s32.astype(np.float64))


def _perm(n, seed):
    return _cached(("perm", n, seed), lambda: np.random.default_rng(seed).permutation(n))


def _sample(dt, n, seed=7):
    """n values of the stress set in a fixed order, the special values first."""
    if dt is np.float16:
        s = _stress(dt)
        return s[_perm(s.size, seed)][:n].copy()
    s = _stress(np.float32)
    head = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                     1.0, -1.0, 0.5, 2.0, 105615.0, 105616.0], dtype=np.float32)
    out = np.concatenate([head, s[_perm(s.size, seed)][:n - head.size]])
    with np.errstate(all="ignore"):
        return out.astype(dt)


def _exact(name):
    """The function in the wide type over the stress set (float32 and float64 share the arguments, hence the reference)."""
    def make():
        with np.errstate(all="ignore"):
            return getattr(np, name)(_stress(np.float32).astype(LD))
    return _cached(("exact", name), make)


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _assert_same_bits(got, ref, what):
    """unsigned bit patterns equal, NaN == NaN"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    eq = _bits(got) == _bits(ref)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(ref)
    if not eq.all():
        i = np.flatnonzero(~eq.ravel())
        raise AssertionError(f"{what}: {i.size} of {eq.size} differ; first at {i[0]}: got {got.ravel()[i[0]]!r} "
                             f"({_bits(got).ravel()[i[0]]:#x}), expected {ref.ravel()[i[0]]!r} ({_bits(ref).ravel()[i[0]]:#x})")


def _ulp_max(dt):
    fi = np.finfo(dt)
    return 2.0 ** (fi.maxexp - 1 - fi.nmant)          # spacing at the largest finite value


def _ulp_errors(x, got, exact, dt, bound, what):
    """Checks the NaN and inf patterns of `got` against T(exact); -> (max error in ulps of T, its argument).
    error = |got - exact| / spacing(|T(exact)|) where T(exact) is finite. Where |exact| lies within `bound` ulps of the overflow
    threshold either answer (the largest finite value or inf) passes."""
    with np.errstate(all="ignore"):
        te = exact.astype(dt)
        um = LD(_ulp_max(dt))
        near = np.abs(np.abs(exact) - (LD(np.finfo(dt).max) + um / 2)) <= bound * um
    assert got.dtype == np.dtype(dt), (what, got.dtype)
    bad = np.isnan(got) != np.isnan(te)
    assert not bad.any(), f"{what}: NaN pattern differs at x = {x[bad][:4]!r}: got {got[bad][:4]!r}, expected {te[bad][:4]!r}"
    bad = ((np.isinf(got) != np.isinf(te)) & ~near) | (np.isinf(got) & np.isinf(te) & (got != te))
    assert not bad.any(), f"{what}: inf pattern differs at x = {x[bad][:4]!r}: got {got[bad][:4]!r}, expected {te[bad][:4]!r}"
    ok = np.isfinite(te) & np.isfinite(got)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(te[ok])).astype(LD)
        sp[~np.isfinite(sp)] = um
        err = np.abs(got[ok].astype(LD) - exact[ok]) / sp
    i = int(np.argmax(err))
    return float(err[i]), x[ok][i]


# -------------------------------------------------------------------------------------------------------- A. accuracy in ulps
def _accuracy(ctx, dt):
    x = _stress(dt)
    dx = nd.asarray(x)
    rows, fails = [], []
    for name in FUNCS:
        got = getattr(nd, name)(dx).get()
        if name == "sqrt":
            with np.errstate(all="ignore"):
                _assert_same_bits(got, np.sqrt(x), f"{dt.__name__} sqrt (correctly rounded)")
        bound = 0.5 if name == "sqrt" else (BOUND_SINCOS32 if dt is np.float32 and name in ("sin", "cos") else BOUND[dt])
        worst, arg = _ulp_errors(x, got, _exact(name), dt, bound, f"{dt.__name__} {name}")
        rows.append(f"{ctx.tag:10s} {dt.__name__:8s} {name:5s} max {worst:7.3f} ulp at x = {arg!r:<24} (bound {bound:g})")
        if worst > bound:
            fails.append(rows[-1])
        z = x == 0
        if name == "sin":
            assert (got[z] == 0).all() and np.array_equal(np.signbit(got[z]), np.signbit(x[z])), "sin(-0.0) is -0.0, sin(+0.0) is +0.0"
        if name == "cos":
            assert (got[z] == 1).all(), "cos(+-0) is 1"
    # float power on a grid: bases in (0, 4], exponents in [-3, 3] without the exponents BPow answers by a shortcut
    a32 = (np.arange(1, 1025, dtype=np.float32) / np.float32(256))
    b32 = np.concatenate([np.arange(-192, 193, dtype=np.float32) / np.float32(64), np.array([1 / 3, -1 / 3, 2.5000002, 0.49999997], np.float32)])
    b32 = b32[~np.isin(b32, np.array([2, 1, 0, 0.5, -1], np.float32))]
    A, B = [v.ravel() for v in np.meshgrid(a32, b32, indexing="ij")]
    exact = _cached("exact_pow", lambda: np.power(A.astype(LD), B.astype(LD)))
    got = nd.power(nd.asarray(A.astype(dt)), nd.asarray(B.astype(dt))).get()
    worst, i = _ulp_errors(np.arange(A.size), got, exact, dt, BOUND[dt], f"{dt.__name__} power")
    rows.append(f"{ctx.tag:10s} {dt.__name__:8s} power max {worst:7.3f} ulp at {dt(A[i])!r} ** {dt(B[i])!r} (bound {BOUND[dt]:g})")
    if worst > BOUND[dt]:
        fails.append(rows[-1])
    ctx.say("\n" + "\n".join(rows))
    assert not fails, "\n".join(fails)


def _accuracy32(ctx):
    """float32 sin cos tan sinh cosh tanh exp log sqrt power against np.longdouble: 4 ulp, sin / cos 2 ulp, sqrt exact."""
    _accuracy(ctx, np.float32)


def _accuracy64(ctx):
    """float64 against np.longdouble: 4 ulp, sqrt exact."""
    if not HAVE_LD:
        pytest.skip("np.longdouble is no wider than float64 here (nmant < 63): no reference for the float64 accuracy tests")
    _accuracy(ctx, np.float64)


test_accuracy_float32_cpu, test_accuracy_float32_gpu = _twin(_accuracy32)
test_accuracy_float64_cpu, test_accuracy_float64_gpu = _twin(_accuracy64)


def _power_shortcuts(ctx):
    """BPow's exponents 2, 1, 0, 0.5, -1 (array exponent) and the unary kernels a host-scalar exponent is dispatched to (USquare, URecip,
    UOne, UPowHalf): bit for bit the correctly rounded power, which NumPy gives as x * x, x, 1, sqrt(x) and 1 / x with C99 pow's special
    cases (pow(-0, .5) = +0, pow(-inf, .5) = +inf, pow(NaN, 0) = 1) — signed zeros, infinities, NaNs and negative bases included.
    (np.power itself is not the reference: NumPy's vectorised float32 power loop is inexact even here — x ** 1.0 != x for 3 of these
    131072 arguments, one ulp off.)"""
    for dt in (np.float32, np.float64):
        x = _sample(dt, 1 << 17)
        dx = nd.asarray(x)
        with np.errstate(all="ignore"):
            half = np.sqrt(x)
            half[x == 0] = 0.0
            half[x == -np.inf] = np.inf
            refs = {2.0: x * x, 1.0: x, 0.0: np.ones_like(x), 0.5: half, -1.0: dt(1) / x}
            # the two patched points are NumPy's own answers (float64 power goes through libm's pow, which follows C99 here)
            patched = (x == 0) | (x == -np.inf)
            _assert_same_bits(half[patched], np.power(x[patched].astype(np.float64), 0.5).astype(dt), f"{dt.__name__} reference of x ** 0.5 at +-0, -inf")
        xs = x[:N_PATH]
        for e, ref in refs.items():
            # the unary kernels behind a host-scalar exponent on the other eager paths (transposed, strided, axes kernels)
            for lay in (_lay_transposed, _lay_strided, _lay_sliced3d):
                _assert_same_bits(nd.power(lay(xs), e).get().ravel(), ref[:N_PATH], f"{dt.__name__} x ** {e}, {lay.__name__[5:]}")
            _assert_same_bits(nd.power(dx, nd.asarray(np.full(x.shape, e, dt))).get(), ref, f"{dt.__name__} x ** array({e})")
            _assert_same_bits(nd.power(dx, e).get(), ref, f"{dt.__name__} x ** {e}")


test_power_shortcuts_cpu, test_power_shortcuts_gpu = _twin(_power_shortcuts)


# ------------------------------------------------------------------------------------------------ B. bit for bit against NumPy
def _f16_subset():
    """2048 float16 patterns: 32 per binade and sign, the first and the last of every binade among them (zeros, the smallest and the
    largest subnormal, the largest finite value, the infinities, NaNs)."""
    k = np.arange(2048)
    off = (k * 11) % 32
    off[k % 32 == 0] = 0
    off[k % 32 == 31] = 31
    return (k * 32 + off).astype(np.uint16).view(np.float16)


def _exact_ops(ctx):
    """absolute negative sign ceil floor sqrt / add subtract multiply true_divide floor_divide mod maximum minimum and the comparisons equal
    NumPy bit for bit (NaN == NaN): subnormals kept, division and square root correctly rounded, NaN-propagating maximum / minimum,
    the sign of zero in mod and floor_divide. float16: both sides compute in float32 and round once."""
    for dt in (np.float32, np.float64, np.float16):
        x = _stress(dt)
        dx = nd.asarray(x)
        with np.errstate(all="ignore"):
            for name in UNARY_EXACT:
                _assert_same_bits(getattr(nd, name)(dx).get(), getattr(np, name)(x), f"{dt.__name__} {name}")
            if dt is np.float16:
                s = _f16_subset()
                a, b = np.repeat(s, s.size), np.tile(s, s.size)          # ~4 M pairs
            else:
                a, b = x, x[_perm(x.size, 11)]
            da, db = nd.asarray(a), nd.asarray(b)
            for name in BINARY_EXACT:
                _assert_same_bits(getattr(nd, name)(da, db).get(), getattr(np, name)(a, b), f"{dt.__name__} {name}")
                if name in ("subtract", "true_divide", "floor_divide", "mod", "less", "greater_equal"):      # the other operand order
                    _assert_same_bits(getattr(nd, name)(db, da).get(), getattr(np, name)(b, a), f"{dt.__name__} {name} (swapped)")


test_exact_ops_cpu, test_exact_ops_gpu = _twin(_exact_ops)


def _f16_transcendentals(ctx):
    """float16 sin .. sqrt over all 65536 patterns: |got - exact| <= spacing(|f16(exact)|) / 2 + 4 spacing(|f32(exact)|) — one float16
    rounding on top of the float32 budget; NaN and inf patterns those of f16(exact). Printed, not asserted: how many results differ
    from the correctly rounded one (NumPy's own loops beside it)."""
    x = _stress(np.float16)
    dx = nd.asarray(x)
    rows = []
    for name in FUNCS:
        got = getattr(nd, name)(dx).get()
        assert got.dtype == np.float16
        with np.errstate(all="ignore"):
            exact = getattr(np, name)(x.astype(np.float64))
            e16, e32 = exact.astype(np.float16), exact.astype(np.float32)
            theirs = getattr(np, name)(x)
            near = np.abs(np.abs(exact) - 65520.0) <= 4 * np.spacing(np.float32(65520.0))
            sp16 = np.spacing(np.abs(e16)).astype(np.float64)
            sp16[np.isinf(sp16)] = 32.0
            lim = sp16 / 2 + 4 * np.spacing(np.abs(e32)).astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(e16)), f"float16 {name}: NaN pattern"
        bad = ((np.isinf(got) != np.isinf(e16)) & ~near) | (np.isinf(got) & np.isinf(e16) & (got != e16))
        assert not bad.any(), f"float16 {name}: inf pattern differs at {x[bad][:4]!r}"
        ok = np.isfinite(e16) & np.isfinite(got)
        viol = ok.copy()
        viol[ok] = np.abs(got[ok].astype(np.float64) - exact[ok]) > lim[ok]
        rows.append(f"{ctx.tag:10s} float16  {name:5s} {int(viol.sum())} violations; differ from the correctly rounded result: "
                    f"{int((_bits(got)[ok] != _bits(e16)[ok]).sum())} here, {int((_bits(theirs)[ok] != _bits(e16)[ok]).sum())} in NumPy's loop")
        assert not viol.any(), f"float16 {name}: beyond the bound at {x[viol][:4]!r}: got {got[viol][:4]!r}, exact {exact[viol][:4]!r}"
    ctx.say("\n" + "\n".join(rows))


test_f16_transcendentals_cpu, test_f16_transcendentals_gpu = _twin(_f16_transcendentals)


# ------------------------------------------------------------------------------------------------ C. one result on every path
N_PATH = 1 << 16          # (8, 32, 256) = (256, 256): large enough for k_ew_axes (>= 2**16) and k_unary_tr (>= 2**14)


def _lay_flat(h):
    return nd.asarray(h)


def _lay_transposed(h):
    return nd.asarray(np.ascontiguousarray(h.reshape(256, 256).T)).T


def _lay_strided(h):
    big = np.zeros(2 * h.size, h.dtype)
    big[::2] = h
    return nd.asarray(big)[::2]


def _lay_sliced3d(h):
    big = np.zeros((8, 34, 264), h.dtype)
    big[:, 1:33, 4:260] = h.reshape(8, 32, 256)
    return nd.asarray(big)[:, 1:33, 4:260]


def _functor_cases(dt):
    """(name, callable on device operands, host operands, result is bool)"""
    x, y = _sample(dt, N_PATH, 7), _sample(dt, N_PATH, 8)
    y = y[_perm(N_PATH, 9)]
    m = (np.random.default_rng(10).integers(0, 2, N_PATH) == 1)
    cases = []
    for name in UNARY_ALL:
        cases.append((name, getattr(nd, name), (x,), name in ("logical_not", "isnan")))
    for name in BINARY_ALL:
        cases.append((name, getattr(nd, name), (x, y), name in BINARY_EXACT[8:] or name.startswith("logical")))
    cases.append(("where", nd.where, (m, x, y), False))
    return cases


def _paths(ctx, dt):
    lazy = dt is not np.float16           # storage-only types are never leaves of a fused program
    # Interpreter legs: which of k_vm_eval_fast / _axes / _generic serves a program is decided by the operands' geometry alone (fusion.hip
    # plan_eval): dense -> fast; a sliced (8, 32, 256) view with aligned rows of 2**16 elements -> axes; a [::2] view (inner stride 2) ->
    # generic. Neither FUSION_STATS nor the C-ABI tells the three apart, so the layouts are chosen by those rules and not asserted.
    scalar = float(dt(0.3))               # exactly representable in dt: a Python float operand means this value in every loop
    for name, f, hs, is_bool in _functor_cases(dt):
        what = f"{dt.__name__} {name}"
        base = f(*[_lay_flat(h) for h in hs]).get()
        assert base.dtype == (np.bool_ if is_bool else dt), (what, base.dtype)

        def same(got, leg, ref=base):
            _assert_same_bits(np.asarray(got).reshape(ref.shape), ref, f"{what}: {leg} against the contiguous eager kernel")

        for nt in (0, 1):
            ctx.mdopt("nt", nt)
            same(f(*[_lay_flat(h) for h in hs]).get(), f"nt = {nt}")
        ctx.mdopt("nt", -1)
        for lay in (_lay_transposed, _lay_strided, _lay_sliced3d):
            same(f(*[lay(h) for h in hs]).get(), lay.__name__[5:])
        if len(hs) > 1:
            # the LAST operand as a (B, 1, C) broadcast and as a host scalar
            yb = hs[-1].reshape(8, 32, 256)[:, :1, :]
            ref_b = f(*[_lay_flat(h) for h in hs[:-1]], _lay_flat(np.ascontiguousarray(np.broadcast_to(yb, (8, 32, 256))).ravel())).get()
            same(f(*[nd.asarray(h.reshape(8, 32, 256)) for h in hs[:-1]], nd.asarray(np.ascontiguousarray(yb))).get(), "(B, 1, C) broadcast", ref_b)
            same(f(*[_lay_sliced3d(h) for h in hs[:-1]], nd.asarray(np.ascontiguousarray(yb))).get(), "sliced view op (B, 1, C) broadcast", ref_b)
            ref_s = f(*[_lay_flat(h) for h in hs[:-1]], _lay_flat(np.full(N_PATH, scalar, dt))).get()
            same(f(*[_lay_flat(h) for h in hs[:-1]], scalar).get(), "scalar operand", ref_s)
        if name != "where" and not is_bool:
            o = nd.asarray(hs[0].copy())
            r = f(o, *[_lay_flat(h) for h in hs[1:]], out=o)
            assert r is o
            same(o.get(), "out= in place")
        if not lazy:
            continue
        prev = nd.set_lazy(True)
        try:
            for jit in ((0, 1) if ctx.on_gpu else (0,)):
                ctx.mdopt("jit", jit)
                ctx.mdopt("jit_min", 1 if jit else 1 << 18)
                for lay in ((_lay_flat,) if jit else (_lay_flat, _lay_sliced3d, _lay_strided)):
                    r = f(*[lay(h) for h in hs])
                    assert r._expr is not None, f"{what}: not recorded in lazy mode"
                    r = nd.logical_and(r, r) if is_bool else nd.multiply(r, 1.0)      # a real two-instruction program (never + 0.0: the sign of a zero)
                    assert r._expr is not None and r._buf is None, f"{what}: program was evaluated early"
                    before = ctx.jit_launched()
                    got = r.get()
                    if jit:
                        assert ctx.jit_launched() > before, f"{what}: the generated kernel did not run"
                    else:
                        assert ctx.jit_launched() == before, f"{what}: jit = 0 ran a generated kernel"
                    same(got, f"lazy, jit = {jit}, {lay.__name__[5:]}")
        finally:
            nd.set_lazy(prev)


def _paths32(ctx):
    """float32: every unary functor, every binary functor and `where` return the bits of the contiguous eager kernel with non-temporal
    accesses on and off, on a transposed, a strided and a sliced 3-D view, under a (B, 1, C) broadcast, with a scalar operand, in place,
    through the interpreter's three kernels, and (device) through the kernel hiprtc generates."""
    _paths(ctx, np.float32)


def _paths64(ctx):
    """float64: as float32."""
    _paths(ctx, np.float64)


def _paths16(ctx):
    """float16 (narrow kernels k_nw_*): the eager paths; storage-only types are never fused."""
    _paths(ctx, np.float16)


test_paths_float32_cpu, test_paths_float32_gpu = _twin(_paths32)
test_paths_float64_cpu, test_paths_float64_gpu = _twin(_paths64)
test_paths_float16_cpu, test_paths_float16_gpu = _twin(_paths16)


# ------------------------------------------------------------------------------------------------------------------ D. chains
def _chain_list(z0):
    """(label, f(mod, x, y, z, m), has a transcendental); `mod` is nd or np, `z0` the zero of the dtype"""
    return [
        ("x*y + z", lambda q, x, y, z, m: q.add(q.multiply(x, y), z), False),
        ("z + x*y", lambda q, x, y, z, m: q.add(z, q.multiply(x, y)), False),
        ("x*y - z", lambda q, x, y, z, m: q.subtract(q.multiply(x, y), z), False),
        ("z - x*y", lambda q, x, y, z, m: q.subtract(z, q.multiply(x, y)), False),
        ("(x + y)*z", lambda q, x, y, z, m: q.multiply(q.add(x, y), z), False),
        ("x*x + y", lambda q, x, y, z, m: q.add(q.multiply(x, x), y), False),
        ("x/y + z", lambda q, x, y, z, m: q.add(q.true_divide(x, y), z), False),
        ("where(m, x*y, 0) + z", lambda q, x, y, z, m: q.add(q.where(m, q.multiply(x, y), z0), z), False),
        ("exp(x)*y + z", lambda q, x, y, z, m: q.add(q.multiply(q.exp(x), y), z), True),
    ]


def _chains(ctx, dt):
    n = 1 << 18
    x, y, z = _sample(dt, n, 21), _sample(dt, n, 22)[_perm(n, 23)], _sample(dt, n, 24)[_perm(n, 25)]
    m = np.random.default_rng(26).integers(0, 2, n) == 1
    # the one-pass "product and column sum" form wants a 2-D shape it serves: 512 x 1024
    R, Cn = 512, 1024
    x2, y2, z2 = [np.concatenate([v, v[_perm(n, 27)]]).reshape(R, Cn) for v in (x, y, z)]
    m2 = np.concatenate([m, ~m]).reshape(R, Cn)
    dx, dy, dz, dm = [nd.asarray(v) for v in (x, y, z, m)]
    dx2, dy2, dz2, dm2 = [nd.asarray(v) for v in (x2, y2, z2, m2)]
    chains = _chain_list(dt(0))
    prev = nd.set_lazy(False)
    try:
        eager, eager2 = [], []
        for label, f, transcendental in chains:
            e = f(nd, dx, dy, dz, dm).get()
            if not transcendental:
                with np.errstate(all="ignore"):
                    _assert_same_bits(e, f(np, x, y, z, m), f"{dt.__name__} {label}: eager against NumPy")
            eager.append(e)
            eager2.append(f(nd, dx2, dy2, dz2, dm2).get())
        nd.set_lazy(True)
        for jit in ((0, 1) if ctx.on_gpu else (0,)):
            ctx.mdopt("jit", jit)
            ctx.mdopt("jit_min", 1 if jit else 1 << 18)
            leg = f"lazy, jit = {jit}"
            for (label, f, _), e, e2 in zip(chains, eager, eager2):
                what = f"{dt.__name__} {label}: {leg}"
                r = f(nd, dx, dy, dz, dm)
                assert r._expr is not None and r._buf is None, what
                before = ctx.jit_launched()
                got = r.get()
                assert (ctx.jit_launched() > before) == bool(jit), f"{what}: generated kernel {'did not run' if jit else 'ran'}"
                _assert_same_bits(got, e, f"{what} against eager")
                # stored elementwise output of the evaluate + column-sum pass (generated kernel; two passes on the interpreter)
                s0 = dict(nd.FUSION_STATS)
                g = f(nd, dx2, dy2, dz2, dm2)
                cs = nd.sum(g, axis=0)
                assert g._expr is not None and g._buf is None, what
                nd.materialize(g)
                if jit:
                    assert nd.FUSION_STATS["vm_eval_reduce_cols"] - s0["vm_eval_reduce_cols"] == 1, f"{what}: no one-pass product + column sum"
                _assert_same_bits(g.get(), e2, f"{what}, stored output of the product + column sum pass, against eager")
                assert cs.get().shape == (Cn,)
            # multi-output: programs that share leaves, evaluated by one call
            for lo in (0, 4, 5):
                s0 = dict(nd.FUSION_STATS)
                before = ctx.jit_launched()
                outs = [f(nd, dx, dy, dz, dm) for _, f, _ in chains[lo:lo + 4]]
                assert all(o._expr is not None for o in outs)
                nd.materialize_many(outs)
                assert nd.FUSION_STATS["vm_eval_multi"] - s0["vm_eval_multi"] == 1, f"{dt.__name__} {leg}: materialize_many did not share a call"
                assert (ctx.jit_launched() > before) == bool(jit)
                for o, (label, _, _), e in zip(outs, chains[lo:lo + 4], eager[lo:lo + 4]):
                    _assert_same_bits(o.get(), e, f"{dt.__name__} {label}: {leg}, materialize_many, against eager")
    finally:
        nd.set_lazy(prev)


def _chains32(ctx):
    """float32 chains x*y + z, z + x*y, x*y - z, z - x*y, (x + y)*z, x*x + y, x/y + z, where(m, x*y, 0) + z, exp(x)*y + z: eager equals
    NumPy bit for bit (the chains without a transcendental); the interpreter, the generated kernels (device), materialize_many and the
    stored output of the one-pass product + column sum equal eager bit for bit — a*b + c rounds twice everywhere."""
    _chains(ctx, np.float32)


def _chains64(ctx):
    """float64: as float32."""
    _chains(ctx, np.float64)


test_chains_float32_cpu, test_chains_float32_gpu = _twin(_chains32)
test_chains_float64_cpu, test_chains_float64_gpu = _twin(_chains64)
