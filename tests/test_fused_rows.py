"""Lazy mode: a pending chain reduced over its TRAILING axes in one pass (mdhip_vm_reduce's third form).

CPU (the test double refuses the row mask): the call is offered with the right mask, the refusal falls back to today's route with
the right values, and shapes outside the form are never offered.

GPU, each case through the generated kernels (options jit = 1, jit_min = 1: exactly one generated launch per reduction) and through
the interpreter kernel (option jit = 0 — at the default threshold the larger shapes here would take the generated kernels in both
legs). References: the SAME chain evaluated eagerly (the functors are bit-identical, only the order of combination differs), then
reduced in NumPy — in the chain's dtype for max / min, in float64 for sums.
  exact      sums of integer-valued products, products of +-2^k factors, max / min of a permutation with an extreme or a NaN
             planted (one run per position): bit for bit, so every element is combined exactly once and lands in its own row
  inexact    |got - ref| <= k u sum|v| per row, k the longest chain of additions in the kernel as built (_chain_length)
  forms      wave per row with 1 / 2 / 4 / 8 vector groups per lane, block per row; every leaf kind; refusals; determinism
  end to end softmax cross-entropy and a (B,R,1) scale through the tape, lazy against eager."""
import ctypes as C
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
f32, f64 = np.dtype(np.float32), np.dtype(np.float64)

NUM_CUS = 256            # MD_NUM_CUS: the floor on the number of long rows (no cross-block split yet)
WAVE_MAX = 64 * 4 * 8    # longest row of the wave-per-row generated kernels: 64 lanes x 8 groups x 4 elements


@pytest.fixture
def lazy_nd(lib):
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(True)
    yield nd
    nd.set_lazy(prev)


@pytest.fixture(params=["generated", "interpreter"])
def generated(request, mdopt):
    """True: the hiprtc-compiled kernels at any size; False: the interpreter kernel k_vm_reduce_rows."""
    mdopt("jit_min", 1)
    mdopt("jit", 1 if request.param == "generated" else 0)
    return request.param == "generated"


_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("MDHIP_FUSED_ROWS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float sums of tests/test_fused_rows.py: largest |got - float64 sum| / (u * sum|v|) over the rows, per form "
                    "(bound k: the longest chain of additions of that form at that row length)\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key][0]:8.3f}  k = {_RATIOS[key][1]:2d}  {key}\n")


def _launched(lib):
    st = (C.c_int64 * 2)()
    lib.vm_jit_stats(st)
    return int(st[1])


def _same(got, exp, what):
    """bit for bit; a NaN matches any NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    gn, en = np.isnan(got), np.isnan(exp)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = (gn != en) | (~en & (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(exp).view(u)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} against {exp[tuple(np.argwhere(bad)[0])]!r}"


def _eager(nd, make):
    prev = nd.set_lazy(False)
    try:
        return make().get()
    finally:
        nd.set_lazy(prev)


def _fused(nd, lib, generated, make, op, axis=-1, keepdims=False, what=""):
    """op(pending chain) over `axis`: one vm_reduce_rows call, one generated launch (or none), the operand stays pending"""
    e = make()
    assert e._expr is not None and e._buf is None, f"{what}: the chain should be pending"
    s0, l0 = nd.FUSION_STATS["vm_reduce_rows"], _launched(lib)
    r = getattr(nd, op)(e, axis=axis, keepdims=keepdims)
    assert nd.FUSION_STATS["vm_reduce_rows"] - s0 == 1, f"{what}: not fused"
    assert _launched(lib) - l0 == (1 if generated else 0), f"{what}: generated kernels launched"
    assert e._buf is None, f"{what}: the reduction materialised its operand"
    return r.get()


def _fallback(nd, make, op, axis, keepdims=False, what=""):
    """the same call where the form does not apply: today's route, vm_reduce_rows unchanged"""
    e = make()
    assert e._expr is not None and e._buf is None, f"{what}: the chain should be pending"
    s0 = nd.FUSION_STATS["vm_reduce_rows"]
    got = getattr(nd, op)(e, axis=axis, keepdims=keepdims).get()
    assert nd.FUSION_STATS["vm_reduce_rows"] == s0, f"{what}: counted as fused"
    return got


def _chain_length(n_red, generated):
    """The longest chain of floating-point additions one element passes through, from the geometry of the kernel as built
    (csrc/fusion.hip k_vm_reduce_rows, csrc/fusion_jit.inc RED_ROWS); the first addition of an accumulator, to the identity, is exact.
      interpreter    a wave per row: lane l takes vector groups l, l + 64, .. in ceil(nvec / 64) trips, alternating between two sets
                     of four accumulators -> ceil(trips / 2) - 1 serial additions, 1 to merge the sets, 2 to merge the four
                     components, 6 levels of the 64-lane tree
      wave per row   (generated, rows up to 2048) ceil(nvec / 64) groups per lane into four accumulators -> groups - 1, then 2 + 6
      block per row  (generated, longer rows) 256 lanes, trips = ceil(nvec / 256) alternating between two sets -> ceil(trips / 2) - 1,
                     then 1 + 2 + 6 and 2 more for the four wave partials"""
    nvec = n_red // 4
    if not generated:
        trips = -(-nvec // 64)
        return -(-trips // 2) - 1 + 1 + 2 + 6
    if n_red <= WAVE_MAX:
        return -(-nvec // 64) - 1 + 2 + 6
    trips = -(-nvec // 256)
    return -(-trips // 2) - 1 + 1 + 2 + 6 + 2


def _form(n_red, generated):
    if not generated:
        return "interpreter, wave per row"
    if n_red > WAVE_MAX:
        return "generated, block per row"
    nvec = n_red // 4
    return f"generated, wave per row, NV = {1 if nvec <= 64 else 2 if nvec <= 128 else 4 if nvec <= 256 else 8}"


def _check_sum(got, v, n_red, generated, what, axis=-1):
    """|got - ref| <= k u sum|v| per row, ref the float64 sum of the eagerly evaluated chain"""
    wide = v.astype(np.float64)
    ref, mass = wide.sum(axis=axis), np.abs(wide).sum(axis=axis)
    u = 2.0 ** (-24 if v.dtype == f32 else -53)
    k = _chain_length(n_red, generated)
    assert k <= min(n_red - 1, 34), (what, k)          # no looser than the eager row kernels (tests/test_reduce_paths.py)
    ratio = float((np.abs(got.astype(np.float64).reshape(ref.shape) - ref) / (u * mass)).max())
    key = f"{_form(n_red, generated)} [n_red = {n_red}, {v.dtype.name}]"
    _RATIOS[key] = (max(ratio, _RATIOS.get(key, (0.0, k))[0]), k)
    print(f"{what}: ratio {ratio:.3f}, k = {k}")
    assert ratio <= k, (what, ratio, k)


# ------------------------------------------------------------------------------------------------------------------ CPU, on the double
def _spy(nd, monkeypatch):
    calls = []
    real = nd._lib().vm_reduce

    def spy(prog, code, shape_like, out, mask):
        calls.append((tuple(shape_like.shape[:shape_like.ndim]), int(mask)))
        return real(prog, code, shape_like, out, mask)

    monkeypatch.setattr(nd._lib(), "vm_reduce", spy)
    return calls


@pytest.mark.parametrize("shape, axis, keepdims, mask", [((64, 256), -1, False, 0b10), ((8, 4, 16), (1, 2), False, 0b110),
                                                         ((64, 256), -1, True, 0b10), ((8, 4, 16), (1, 2), True, 0b110)])
def test_row_mask_is_offered_and_the_refusal_falls_back_cpu(lazy_nd, on_gpu, monkeypatch, shape, axis, keepdims, mask):
    """The double refuses the trailing-axis mask: the call must have been made (it is not on the parent commit), the result is
    that of today's route — one materialisation of the operand, then the eager reduction — and nothing is counted as fused."""
    if on_gpu:
        pytest.skip("other twin")
    nd = lazy_nd
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    dx, dy = nd.asarray(x), nd.asarray(y)
    calls = _spy(nd, monkeypatch)
    s0 = dict(nd.FUSION_STATS)
    e = nd.multiply(dx, dy)
    assert e._expr is not None and e._buf is None
    r = nd.sum(e, axis=axis, keepdims=keepdims)
    assert calls == [(shape, mask)], calls
    ref = (x.astype(np.float64) * y).sum(axis=axis, keepdims=keepdims)
    got = r.get()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    assert nd.FUSION_STATS["vm_reduce_rows"] == s0["vm_reduce_rows"] and nd.FUSION_STATS["vm_reduce"] == s0["vm_reduce"]
    assert e._buf is not None and nd.FUSION_STATS["vm_eval"] - s0["vm_eval"] == 1      # materialised, once
    assert np.array_equal(e.get(), x * y) and nd.FUSION_STATS["vm_eval"] - s0["vm_eval"] == 1


def test_shapes_outside_the_form_are_never_offered_cpu(lazy_nd, on_gpu, monkeypatch):
    if on_gpu:
        pytest.skip("other twin")
    nd = lazy_nd
    rng = np.random.default_rng(2)
    calls = _spy(nd, monkeypatch)
    x = rng.standard_normal((64, 10)).astype(np.float32)
    got = nd.sum(nd.multiply(nd.asarray(x), 2.0), axis=-1).get()                        # rows of 10: no whole groups of four
    assert np.allclose(got, (x * 2).sum(axis=-1), rtol=1e-5, atol=1e-5)
    xi = rng.integers(-5, 5, (16, 8))
    assert np.array_equal(nd.sum(nd.multiply(nd.asarray(xi), 3), axis=-1).get(), (xi * 3).sum(axis=-1))    # an int64 chain
    x3 = rng.standard_normal((4, 8, 16)).astype(np.float32)
    got = nd.sum(nd.multiply(nd.asarray(x3), 2.0), axis=(0, 2)).get()                   # a kept axis behind the first reduced one
    assert np.allclose(got, (x3 * 2).sum(axis=(0, 2)), rtol=1e-5, atol=1e-5)
    xb = rng.standard_normal((16, 8)).astype(np.float32)
    m = nd.greater(nd.asarray(xb), 0)                                                   # a bool-valued chain (summed as int64)
    assert m._expr is not None
    assert np.array_equal(nd.sum(m, axis=-1).get(), (xb > 0).sum(axis=-1))
    assert calls == [], calls


# ------------------------------------------------------------------------------------------------------------------------ GPU: exact
# (n_red, n_out): every row length of {one vector, NV = 1 / 2 / 4 / 8 full, each plus one vector, block form, block form with a tail}
# and every form with both row counts: the floor for long rows (NUM_CUS, a multiple of 4) and 1027 (the last block has idle waves)
PAIRS = [(4, 1027), (32, NUM_CUS), (256, 1027), (260, NUM_CUS), (260, 1027), (512, 1027), (516, 1027), (1024, NUM_CUS),
         (1028, NUM_CUS), (1028, 1027), (2048, 1027), (2052, NUM_CUS), (2052, 1027), (8196, NUM_CUS)]


def _positions(n_red):
    """element 0, the last one, and both sides of: the first and the last vector boundary, the lane trip (64 lanes x 4 elements =
    the next vector group of a lane, NV boundary of the wave form), NV = 2 / 4 / 8 limits, the block form's trip (256 lanes x 4)
    and its pair of trips in flight"""
    pos = {0, n_red - 1}
    for b in (4, 256, 512, 1024, 2048, n_red - 4):
        if 0 < b < n_red:
            pos |= {b - 1, b}
    return sorted(pos)


def _rows(n_out):
    """first row, last row of the first block, last row of the last full block, last row"""
    return sorted({0, 3, (n_out // 4) * 4 - 1, n_out - 1})


@gpu
@pytest.mark.parametrize("n_red, n_out", PAIRS)
def test_exact_rows_gpu(lazy_nd, lib, on_gpu, generated, n_red, n_out):
    nd = lazy_nd
    assert on_gpu
    rng = np.random.default_rng(1000 * n_red + n_out)
    for dt in (f32, f64):
        what = f"({n_out}, {n_red}) {dt.name} {_form(n_red, generated)}"
        # sum of x * y, small integers: every partial sum is exact in float32 (|row sum| <= 16 * 8196 < 2^24)
        x = rng.integers(-4, 5, (n_out, n_red)).astype(dt)
        y = rng.integers(-4, 5, (n_out, n_red)).astype(dt)
        dx, dy = nd.asarray(x), nd.asarray(y)
        make = lambda: nd.multiply(dx, dy)              # noqa: E731
        ref = _eager(nd, make).sum(axis=-1, dtype=np.float64).astype(dt)
        _same(_fused(nd, lib, generated, make, "sum", what=what), ref, f"{what}: sum")
        _same(_fused(nd, lib, generated, make, "sum", keepdims=True, what=what), ref.reshape(n_out, 1), f"{what}: sum, keepdims")
        # .. one element changed: exactly one output changes
        r, c = n_out // 2, n_red - 3
        dx[r:r + 1, c:c + 1] = float(x[r, c] + 7)
        exp = ref.copy()
        exp[r] += 7 * y[r, c]
        _same(_fused(nd, lib, generated, make, "sum", what=what), exp, f"{what}: sum, one element changed")
        # prod of +-2^k factors: signs in x; y holds 12 twos and 5 halves per row (fewer in short rows), ones elsewhere — any
        # partial product stays within 2^+-12
        x = rng.choice(np.array([-1.0, 1.0]), (n_out, n_red)).astype(dt)
        y = np.ones((n_out, n_red), dt)
        n2, nh = min(12, n_red // 2), min(5, n_red // 4)
        for i in range(n_out):
            p = rng.permutation(n_red)[:n2 + nh]
            y[i, p[:n2]], y[i, p[n2:]] = 2.0, 0.5
        dx, dy = nd.asarray(x), nd.asarray(y)
        ref = np.prod(_eager(nd, make).astype(np.float64), axis=-1).astype(dt)
        assert np.all(np.abs(ref) == 2.0 ** (n2 - nh))
        _same(_fused(nd, lib, generated, make, "prod", what=what), ref, f"{what}: prod")
        # max / min of twice a permutation, then an extreme or a NaN planted: one run per position and row
        x = (rng.permutation(n_out * n_red).reshape(n_out, n_red) - n_out * n_red // 2).astype(dt)   # (exact: < 2^23)
        y = np.full((n_out, n_red), 2.0, dt)
        dx, dy = nd.asarray(x), nd.asarray(y)
        v = _eager(nd, make)
        base = {"max": v.max(axis=-1), "min": v.min(axis=-1)}
        for op in ("max", "min"):
            _same(_fused(nd, lib, generated, make, op, what=what), base[op], f"{what}: {op}, permutation")
        big = float(2 ** 25)
        for r in _rows(n_out):
            for c in _positions(n_red):
                for op, plant in (("max", big), ("min", -big), ("max", np.nan), ("min", np.nan)):
                    dx[r:r + 1, c:c + 1] = plant
                    exp = base[op].copy()
                    exp[r] = dt.type(plant) * dt.type(2.0)
                    _same(_fused(nd, lib, generated, make, op, what=what), exp, f"{what}: {op}, {plant} planted at ({r}, {c})")
                dx[r:r + 1, c:c + 1] = float(x[r, c])
        for op in ("max", "min"):                        # (everything was put back)
            _same(_fused(nd, lib, generated, make, op, what=what), base[op], f"{what}: {op}, restored")


# ------------------------------------------------------------------------------------------------------------------- GPU: leaf kinds
def _leaf_case(nd, name, dt, rng):
    """-> (make, axis, n_red, prod_make): the chain, the reduced axes, the row length; prod_make: a chain of factors near 1"""
    f = lambda *s: rng.standard_normal(s).astype(dt)                 # noqa: E731
    near1 = lambda *s: (1 + 0.01 * rng.standard_normal(s)).astype(dt)   # noqa: E731
    if name == "dense x dense":
        x, y, p = nd.asarray(f(1027, 516)), nd.asarray(f(1027, 516)), nd.asarray(near1(1027, 516))
        return (lambda: nd.multiply(x, y)), -1, 516, (lambda: nd.multiply(p, 1.0))
    if name == "per-row scalar":                                      # exp(x - m), m of shape (R, 1)
        xh = f(1027, 516)
        x, m = nd.asarray(xh), nd.asarray(xh.max(axis=-1, keepdims=True))
        return (lambda: nd.exp(nd.subtract(x, m))), -1, 516, (lambda: nd.exp(nd.multiply(nd.subtract(x, m), 1e-4)))
    if name == "row-invariant vector":                                # a (C,) weight
        x, w, p = nd.asarray(f(1027, 516)), nd.asarray(f(516)), nd.asarray(near1(516))
        return (lambda: nd.multiply(x, w)), -1, 516, (lambda: nd.multiply(nd.add(nd.multiply(x, 0.0), 1.0), p))
    if name == "0-d constant and scalar":
        x, c, p = nd.asarray(f(1027, 516)), nd.asarray(dt.type(0.375)), nd.asarray(near1(1027, 516))
        return (lambda: nd.add(nd.multiply(x, c), 1.5)), -1, 516, (lambda: nd.multiply(nd.multiply(p, c), 1.0 / 0.375))
    if name == "row-sliced operand":                                  # the row stride (1024) is not n_red (512)
        x, y = nd.asarray(f(300, 1024))[:, :512], nd.asarray(f(300, 512))
        p = nd.asarray(near1(300, 1024))[:, :512]
        return (lambda: nd.multiply(x, y)), -1, 512, (lambda: nd.multiply(p, 1.0))
    if name == "3-D, (B,R,1) and (C,)":
        x, m, w = nd.asarray(f(6, 50, 128)), nd.asarray(f(6, 50, 1)), nd.asarray(f(128))
        p, q = nd.asarray(near1(6, 50, 1)), nd.asarray(near1(128))
        return (lambda: nd.multiply(nd.subtract(x, m), w)), -1, 128, (lambda: nd.multiply(nd.add(nd.multiply(x, 0.0), p), q))
    if name == "(B,1,1) under axis=(1,2)":
        x, s, p = nd.asarray(f(40, 8, 64)), nd.asarray(f(40, 1, 1)), nd.asarray(near1(40, 8, 64))
        return (lambda: nd.multiply(x, s)), (1, 2), 512, (lambda: nd.multiply(p, nd.asarray(np.ones((40, 1, 1), dt))))
    raise KeyError(name)


LEAF_KINDS = ["dense x dense", "per-row scalar", "row-invariant vector", "0-d constant and scalar", "row-sliced operand",
              "3-D, (B,R,1) and (C,)", "(B,1,1) under axis=(1,2)"]


@gpu
@pytest.mark.parametrize("kind", LEAF_KINDS)
def test_leaf_kinds_gpu(lazy_nd, lib, on_gpu, generated, kind):
    """Every leaf kind the form reads, all four reductions: max / min bit for bit, sums within the chain-length bound, products
    within the n_red - 1 roundings of a product of factors near 1 taken in any order (relative error <= 1.01 (n_red - 1) u against
    the long-double product of the eagerly evaluated factors)."""
    nd = lazy_nd
    assert on_gpu
    for dt in (f32, f64):
        make, axis, n_red, prod_make = _leaf_case(nd, kind, dt, np.random.default_rng(sum(map(ord, kind))))
        what = f"{kind}, {dt.name}, {_form(n_red, generated)}"
        v = _eager(nd, make)
        for keepdims in (False, True):
            _check_sum(_fused(nd, lib, generated, make, "sum", axis, keepdims, what), v, n_red, generated, f"{what}: sum", axis)
        _same(_fused(nd, lib, generated, make, "max", axis, what=what), v.max(axis=axis), f"{what}: max")
        _same(_fused(nd, lib, generated, make, "min", axis, True, what), v.min(axis=axis, keepdims=True), f"{what}: min, keepdims")
        pv = _eager(nd, prod_make)
        ref = np.prod(pv.astype(np.longdouble), axis=axis)
        got = _fused(nd, lib, generated, prod_make, "prod", axis, what=what)
        u = 2.0 ** (-24 if dt == f32 else -53)
        assert np.all(np.abs(got - ref) <= 1.01 * (n_red - 1) * u * np.abs(ref)), f"{what}: prod"


@gpu
@pytest.mark.parametrize("shape", [(1027, 516), (300, 8196)])
def test_inexact_sums_gpu(lazy_nd, lib, on_gpu, generated, shape):
    nd = lazy_nd
    assert on_gpu
    for dt in (f32, f64):
        rng = np.random.default_rng(shape[1])
        x, y = nd.asarray(rng.standard_normal(shape).astype(dt)), nd.asarray(rng.standard_normal(shape).astype(dt))
        make = lambda: nd.multiply(x, y)                # noqa: E731
        what = f"{shape} {dt.name} {_form(shape[1], generated)}"
        _check_sum(_fused(nd, lib, generated, make, "sum", what=what), _eager(nd, make), shape[1], generated, what)


# -------------------------------------------------------------------------------------------------------- GPU: refusals, determinism
@gpu
def test_refusals_fall_back_gpu(lazy_nd, lib, on_gpu, generated):
    nd = lazy_nd
    assert on_gpu
    rng = np.random.default_rng(7)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)          # noqa: E731
    x10 = nd.asarray(f(64, 10))
    x3, b3 = nd.asarray(f(6, 50, 128)), nd.asarray(f(6, 1, 128))
    xt, yt = nd.asarray(f(256, 128)), nd.asarray(f(128, 256))
    few = nd.asarray(f(NUM_CUS - 4, 4096))
    cases = [("ragged rows", lambda: nd.multiply(x10, 2.0), -1),
             ("(B,1,C) under (B,R,C)", lambda: nd.multiply(x3, b3), -1),
             ("a transposed leaf", lambda: nd.multiply(xt, yt.T), -1),
             ("long rows, fewer than the floor", lambda: nd.multiply(few, 2.0), -1)]
    for what, make, axis in cases:
        v = _eager(nd, make)
        got = _fallback(nd, make, "sum", axis, what=what)
        ref = v.sum(axis=axis, dtype=np.float64)
        assert np.abs(got - ref).max() <= 34 * 2.0 ** -24 * np.abs(v).sum(axis=axis, dtype=np.float64).max(), what
        _same(_fallback(nd, make, "max", axis, what=what), v.max(axis=axis), f"{what}: max")
    # the floor itself is admitted
    at = nd.asarray(f(NUM_CUS, 4096))
    make = lambda: nd.multiply(at, 2.0)                 # noqa: E731
    _same(_fused(nd, lib, generated, make, "max", what="floor"), _eager(nd, make).max(axis=-1), "long rows at the floor: max")


@gpu
def test_deterministic_gpu(lazy_nd, lib, on_gpu, generated):
    """The order of combination is the geometry's: three interleaved repeats of two shapes give the same bits."""
    nd = lazy_nd
    assert on_gpu
    rng = np.random.default_rng(11)
    makes = []
    for shape in ((1027, 516), (NUM_CUS, 2052)):
        x, y = nd.asarray(rng.standard_normal(shape).astype(np.float32)), nd.asarray(rng.standard_normal(shape).astype(np.float32))
        makes.append(lambda x=x, y=y: nd.multiply(nd.exp(x), y))
    first = [_fused(nd, lib, generated, m, "sum") for m in makes]
    for _ in range(2):
        for m, ref in zip(makes, first):
            _same(_fused(nd, lib, generated, m, "sum"), ref, "repeat")


# ----------------------------------------------------------------------------------------------------------------- GPU: end to end
@gpu
def test_softmax_cross_entropy_and_scale_gradient_gpu(lazy_nd, lib, on_gpu, generated):
    """Softmax cross-entropy on (256, 64) logits through the tape: max, exp(x - m), the row sum, log, the row sum of y * logp, the
    mean — loss and logits' gradient in lazy mode against eager mode. (The row sums are taken without keepdims and reshaped: the
    tape's gradient of `sum` tiles a gradient of the reduced shape, as the project it mirrors does; the keepdims form is what
    `unbroadcast` issues for the (4,32,1) scale below.)"""
    nd = lazy_nd
    assert on_gpu
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    md = build_engine(HipBackendTable, "lazy")
    R, Cn = 256, 64

    def sweep(dt):
        rng = np.random.default_rng(3)
        x = (rng.standard_normal((R, Cn)) * 3).astype(dt)
        y = np.zeros((R, Cn), dt)
        y[np.arange(R), rng.integers(0, Cn, R)] = 1
        X, Y = md.Tensor(x, allow_grad=True), md.Tensor(y)
        m = md.Tensor(nd.max(X._data, axis=-1, keepdims=True))
        z = X - m
        s = md.sum(md.exp(z), axis=(1,)).reshape((R, 1))
        logp = z - md.log(s)
        loss = md.sum(md.sum(Y * logp, axis=(1,))) / (-R)
        loss.backward()
        return loss.as_numpy().astype(np.float64), X.grad.as_numpy().astype(np.float64), x.astype(np.float64), y

    for dt, tol in ((f32, 1e-6), (f64, 1e-13)):
        nd.set_lazy(False)
        l_e, g_e, x, y = sweep(dt)
        nd.set_lazy(True)
        s0 = nd.FUSION_STATS["vm_reduce_rows"]
        l_l, g_l, _, _ = sweep(dt)
        assert nd.FUSION_STATS["vm_reduce_rows"] - s0 >= 2, "the two forward row sums"
        assert abs(l_l - l_e) <= tol * abs(l_e), (dt, l_l, l_e)
        assert np.linalg.norm(g_l - g_e) <= tol * np.linalg.norm(g_e), (dt, np.linalg.norm(g_l - g_e) / np.linalg.norm(g_e))
        zz = x - x.max(axis=1, keepdims=True)                        # and both are the softmax's
        lp = zz - np.log(np.exp(zz).sum(axis=1, keepdims=True))
        assert np.linalg.norm(g_e - (np.exp(lp) - y) / R) <= (1e-5 if dt == f32 else 1e-12) * np.linalg.norm((np.exp(lp) - y) / R)

    # d/ds sum(x * s), s of shape (4, 32, 1): unbroadcast issues sum(g * x, axis=-1, keepdims=True) on the pending product
    rng = np.random.default_rng(4)
    x, s = rng.standard_normal((4, 32, 64)).astype(np.float32), rng.standard_normal((4, 32, 1)).astype(np.float32)
    X, S = md.Tensor(x, allow_grad=True), md.Tensor(s, allow_grad=True)
    s0 = nd.FUSION_STATS["vm_reduce_rows"]
    md.sum(X * S).backward()
    g = S.grad.as_numpy()
    assert nd.FUSION_STATS["vm_reduce_rows"] - s0 == 1
    ref = x.astype(np.float64).sum(axis=-1, keepdims=True)
    assert g.shape == (4, 32, 1) and np.linalg.norm(g - ref) <= 1e-6 * np.linalg.norm(ref)
