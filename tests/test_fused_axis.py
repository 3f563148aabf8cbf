"""Lazy mode: a pending chain reduced over a MIDDLE axis (or its leading axes) in one pass — mdhip_vm_reduce's fourth form,
DESIGN.md §4.7: one run of adjacent reduced axes with kept axes behind it, the program seen as (outer, n_red, inner).

CPU (the test double refuses the mask): the call is offered with the right mask, the refusal falls back to today's route with the
right values, shapes outside the form or under its floors are never offered, and probe kinds 8 / 9 compile the two generated
kernels for gfx950.

GPU, each case through the generated kernels (options jit = 1, jit_min = 1: exactly one generated launch per reduction) and through
the interpreter (jit = 0). References: the SAME chain evaluated eagerly, then reduced in NumPy — in the chain's dtype for max / min,
in long double for sums (NumPy adds along a middle axis serially: a float64 accumulator would round as often as the kernels). The kernels as built (csrc/fusion_jit.inc, csrc/fusion.hip), n_red the reduced extent:
  strips       generated, n_red >= 512: NS strips of 256 columns x NB row bands per batch; wave w of band b takes rows
               b + NB (w + 4 i), RU rows per trip, two trips in flight, a tail loop of single rows; the four waves merge in wave
               order, the bands in band order (wave w adds partial rows w, w + 4, ..)
  tiled        generated, n_red < 512: lane row ry takes rows ry + 4 i, even i into one accumulator and odd i into another
               (two rows in flight), a tail of single rows; the two merge, then the four lane rows in a tree
  interpreter  k_vm_reduce_cols, batched: lane row ry takes rows ry + 4 i into one accumulator; the four lane rows in a tree
A reduction of the leading axes (outer = 1) is the 2-D column problem itself and must give its bits."""
import ctypes as C
import os

import numpy as np
import pytest

from minidiff_amd import _capi

gpu = pytest.mark.gpu
f32, f64 = np.dtype(np.float32), np.dtype(np.float64)

NUM_CUS = 256            # MD_NUM_CUS
TICKET_PAD, TICKET_WORDS = 16, 16384
STRIPS_MIN_RED = 512     # sweep_geometry's floor; below it the tiled form
CODES = {"sum": _capi.R_SUM, "prod": _capi.R_PROD, "max": _capi.R_MAX, "min": _capi.R_MIN}


@pytest.fixture
def lazy_nd(lib):
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(True)
    yield nd
    nd.set_lazy(prev)


@pytest.fixture(params=["generated", "interpreter"])
def generated(request, mdopt):
    """True: the hiprtc-compiled kernels at any size; False: the interpreter kernel k_vm_reduce_cols."""
    mdopt("jit_min", 1)
    mdopt("jit", 1 if request.param == "generated" else 0)
    return request.param == "generated"


_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("MDHIP_FUSED_AXIS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float sums of tests/test_fused_axis.py: largest |got - long-double sum| / (u * sum|v|) over the outputs, per form "
                    "(bound k: the longest chain of additions of that form at that geometry)\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key][0]:8.3f}  k = {_RATIOS[key][1]:3d}  {key}\n")


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


def _mask(axis, ndim):
    axes = (axis,) if isinstance(axis, int) else tuple(axis)
    m = 0
    for a in axes:
        m |= 1 << (a % ndim)
    return m


def _fused(nd, lib, generated, make, op, axis=1, keepdims=False, what=""):
    """op(pending chain) over `axis`: one vm_reduce_axis call, one generated launch (or none), the operand stays pending. Shapes under
    the floors of _fused_reduce go to mdhip_vm_reduce through the C-ABI directly (the library has no floors of its own)."""
    e = make()
    assert e._expr is not None and e._buf is None, f"{what}: the chain should be pending"
    mask = _mask(axis, e.ndim)
    s0, l0 = nd.FUSION_STATS["vm_reduce_axis"], _launched(lib)
    if nd._axis_run(e.shape, mask):
        r = getattr(nd, op)(e, axis=axis, keepdims=keepdims)
    else:
        kshape = tuple(1 if (mask >> i) & 1 else n for i, n in enumerate(e.shape))
        r = nd.DeviceArray.empty(kshape, e.dtype)
        prog, keep = nd._lz.build_program(e._expr, e.shape)
        like = nd.ArrayDesc()
        like.dtype, like.ndim = e._expr.cdt, e.ndim
        like.shape[:e.ndim] = e.shape
        lib.vm_reduce(prog, CODES[op], like, r.desc(), mask)       # a refusal raises, with the library's message
        del keep
        nd.FUSION_STATS["vm_reduce_axis"] += 1
        if not keepdims:
            r = r.reshape(tuple(n for i, n in enumerate(e.shape) if not (mask >> i) & 1))
    assert nd.FUSION_STATS["vm_reduce_axis"] - s0 == 1, f"{what}: not fused"
    assert _launched(lib) - l0 == (1 if generated else 0), f"{what}: generated launches {_launched(lib) - l0}"
    assert e._buf is None, f"{what}: the reduction materialised its operand"
    return r.get()


def _fallback(nd, make, op, axis, keepdims=False, what=""):
    """the same call where the library refuses the leaves: today's route, vm_reduce_axis unchanged"""
    e = make()
    assert e._expr is not None and e._buf is None, f"{what}: the chain should be pending"
    s0 = nd.FUSION_STATS["vm_reduce_axis"]
    got = getattr(nd, op)(e, axis=axis, keepdims=keepdims).get()
    assert nd.FUSION_STATS["vm_reduce_axis"] == s0, f"{what}: counted as fused"
    return got


# ------------------------------------------------------------------------------------------------------- the kernels' geometry, as built
def _ru(vec_itemsizes):
    """rows per trip of the strips kernel (sweep_cols): ~128 B of loads in flight per lane over the unit-stride, row-varying leaves"""
    row_bytes = 4 * sum(vec_itemsizes)
    return max(1, min(8, -(-128 // row_bytes))) if row_bytes else 1


def _nb(outer, n_red, inner, ru, forced=0):
    """row bands of the strips kernel (sweep_geometry with `outer` batches)"""
    nse = -(-inner // 256) * outer
    nb = forced if forced > 0 else (1 if nse >= NUM_CUS else NUM_CUS // nse)
    nb = max(1, min(nb, 64, n_red // (4 * ru)))
    if nb > 1 and nse * TICKET_PAD > TICKET_WORDS:
        nb = 1
    return nb


def _form(n_red, generated):
    return "interpreter" if not generated else "strips" if n_red >= STRIPS_MIN_RED else "tiled"


def _chain_length(n_red, form, nb=1):
    """The longest chain of floating-point additions one element passes through; the first addition of an accumulator, to the
    identity, is exact.
      strips       a wave adds its ceil(n_red / (4 NB)) rows into ONE accumulator per column, whatever RU (-> rows - 1), wave 0 adds
                   the other three in turn (3); with bands, wave w adds ceil(NB / 4) partial rows in turn (-> that - 1), then 3 again.
                   This is the 2-D strips kernel's own order: the batch only moves the bases.
      tiled        lane row 0 has ceil(n_red / 4) rows, every second one per accumulator (-> ceil(rows / 2) - 1), 1 to merge the
                   two, 2 levels of the tree over the four lane rows
      interpreter  ceil(n_red / 4) rows into one accumulator (-> rows - 1), 2 levels of the tree"""
    if form == "strips":
        k = -(-n_red // (4 * nb)) - 1 + 3
        return k + (-(-nb // 4) - 1 + 3 if nb > 1 else 0)
    rows = -(-n_red // 4)
    if form == "tiled":
        return max(-(-rows // 2) - 1, 0) + 1 + 2
    return rows - 1 + 2


def _check_sum(got, v, axis, form, nb, what):
    """|got - ref| <= k u sum|v| per output, ref the sum of the eagerly evaluated chain. NumPy adds the rows of a middle axis one
    after the other (no pairwise tree off the contiguous axis), so a float64 accumulator would carry up to n_red - 1 roundings of its
    own — as many as the kernels under test; the reference accumulates in long double (64-bit significand) instead."""
    wide = v.astype(np.longdouble)
    ref, mass = wide.sum(axis=axis), np.abs(wide).sum(axis=axis)
    n_red = int(np.prod([v.shape[a] for a in ((axis,) if isinstance(axis, int) else axis)]))
    u = 2.0 ** (-24 if v.dtype == f32 else -53)
    k = _chain_length(n_red, form, nb)
    ratio = float((np.abs(got.astype(np.longdouble).reshape(ref.shape) - ref) / (u * mass)).max())
    key = f"{form}{f', NB = {nb}' if form == 'strips' else ''} [n_red = {n_red}, {v.dtype.name}]"
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


@pytest.mark.parametrize("op, gshape, axis, keepdims, mask", [("sum", None, 1, False, 0b010), ("sum", None, 1, True, 0b010),
                                                              ("max", None, 1, False, 0b010), ("sum", (8, 1, 256), 1, True, 0b010),
                                                              ("sum", None, (0, 1), False, 0b011)])
def test_axis_mask_is_offered_and_the_refusal_falls_back_cpu(lazy_nd, on_gpu, monkeypatch, op, gshape, axis, keepdims, mask):
    """The double refuses the mask: the call must have been made (it is not on the parent commit), the result is that of today's
    route — one materialisation of the operand, then the eager reduction — and nothing is counted as fused."""
    if on_gpu:
        pytest.skip("other twin")
    nd = lazy_nd
    shape = (8, 64, 256)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(gshape or shape).astype(np.float32)
    dx, dy = nd.asarray(x), nd.asarray(y)
    calls = _spy(nd, monkeypatch)
    s0 = dict(nd.FUSION_STATS)
    e = nd.multiply(dx, dy)
    assert e._expr is not None and e._buf is None
    r = getattr(nd, op)(e, axis=axis, keepdims=keepdims)
    assert calls == [(shape, mask)], calls
    ref = getattr(x.astype(np.float64) * y, op)(axis=axis, keepdims=keepdims)
    got = r.get()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    for key in ("vm_reduce", "vm_reduce_rows", "vm_reduce_axis"):
        assert nd.FUSION_STATS[key] == s0[key], key
    assert e._buf is not None and nd.FUSION_STATS["vm_eval"] - s0["vm_eval"] == 1      # materialised, once
    assert np.array_equal(e.get(), x * y) and nd.FUSION_STATS["vm_eval"] - s0["vm_eval"] == 1


def test_shapes_outside_the_form_are_never_offered_cpu(lazy_nd, on_gpu, monkeypatch):
    if on_gpu:
        pytest.skip("other twin")
    nd = lazy_nd
    rng = np.random.default_rng(2)
    calls = _spy(nd, monkeypatch)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)          # noqa: E731

    def check(x, axis):
        got = nd.sum(nd.multiply(nd.asarray(x), 2.0), axis=axis).get()
        assert np.allclose(got, (x * 2).sum(axis=axis), rtol=1e-4, atol=1e-4)

    check(f(4, 8, 16), (0, 2))                                        # two separated runs
    check(f(4, 64, 512), (0, 2))                                      # .. above the floors as well: the middle axis is kept
    check(f(4, 8, 10), 1)                                             # ragged inner
    check(f(4, 64, 258), 1)                                           # .. above the floors
    xi = rng.integers(-5, 5, (4, 64, 256))
    assert np.array_equal(nd.sum(nd.multiply(nd.asarray(xi), 3), axis=1).get(), (xi * 3).sum(axis=1))    # an int64 chain
    xb = f(4, 64, 256)
    m = nd.greater(nd.asarray(xb), 0)                                 # a bool-valued chain (summed as int64)
    assert m._expr is not None
    assert np.array_equal(nd.sum(m, axis=1).get(), (xb > 0).sum(axis=1))
    check(f(4, 63, 256), 1)                                           # under the floors: n_red
    check(f(4, 64, 252), 1)                                           # .. inner
    check(f(1, 63, 256), (0, 1))                                      # .. the leading-axes route has the same ones
    # outer > 65535: at the floors that is 2^30 elements and more, so the floors are lowered for this one case — the batch alone keeps it away
    monkeypatch.setattr(nd, "_AXIS_MIN_INNER", 4)
    monkeypatch.setattr(nd, "_AXIS_MIN_RED", 2)
    check(f(65536, 2, 4), 1)
    assert calls == [], calls
    check(f(65535, 2, 4), 1)
    assert calls == [((65535, 2, 4), 0b010)], calls
    monkeypatch.undo()
    assert nd._axis_run((65535, 64, 256), 0b010) and not nd._axis_run((65536, 64, 256), 0b010)
    assert nd._axis_run((2, 3, 64, 1, 16, 16), 0b001100) and not nd._axis_run((2, 64, 2, 64, 256), 0b01010)
    assert not nd._axis_run((65536, 256), 0b01) and not nd._axis_run((2, 65536, 256), 0b011) and nd._axis_run((2, 65536, 512), 0b011)


@pytest.fixture(scope="module")
def product():
    if not os.path.exists(_capi.PRODUCT_LIB):
        pytest.skip("libmdhip.so not built")
    lib = _capi.Library(_capi.PRODUCT_LIB)  # dlopen only; the compile-only probe needs no GPU
    return lib, C.create_string_buffer(4096)


UNARY = ["absolute", "sign", "ceil", "floor", "sin", "cos", "tan", "sinh", "cosh", "tanh", "exp", "log", "sqrt", "logical_not",
         "negative", "isnan"]
BINARY = ["add", "subtract", "multiply", "true_divide", "power", "mod", "floor_divide", "maximum", "minimum", "less", "less_equal",
          "greater", "greater_equal", "equal", "not_equal", "logical_and", "logical_or", "logical_xor"]
KINDS = {8: b"k_fused_sweepb_", 9: b"k_fused_redcolsb_"}


def _probe_programs(nd):
    """3-D programs whose axis 1 is the reduced one: the sizes do not matter to the probe, the descriptors do. Operators are chained
    (the generator emits one statement per instruction), so that a handful of compilations covers them all."""
    from minidiff_amd import lazy as lz
    rng = np.random.default_rng(0)
    f = lambda *s: nd.asarray(rng.standard_normal(s).astype(np.float32))   # noqa: E731
    x, y, g, h = f(2, 3, 8), f(2, 3, 8), f(2, 1, 8), f(1, 3, 1)
    arrs = []
    for lo in range(0, len(UNARY), 8):
        acc = nd.multiply(x, g)
        for name in UNARY[lo:lo + 8]:
            acc = nd.add(getattr(nd, name)(acc), 0.5)
        arrs.append((f"unary {lo}..", acc))
    for lo in range(0, len(BINARY), 6):
        acc = nd.add(x, g)
        for name in BINARY[lo:lo + 6]:
            acc = getattr(nd, name)(2.0, nd.add(getattr(nd, name)(acc, y), h))     # a leaf, a stack value and a constant on the left
        arrs.append((f"binary {lo}..", acc))
    m = nd.asarray(rng.integers(0, 2, (2, 1, 8)).astype(bool))
    arrs.append(("where", nd.where(nd.greater(nd.multiply(x, g), 0), nd.multiply(x, m), 0.25)))
    xd, gi = nd.asarray(rng.standard_normal((2, 3, 8))), nd.asarray(rng.integers(-3, 3, (2, 1, 8)))
    arrs.append(("f64 + int64 leaf", nd.add(nd.exp(xd), gi)))
    # every leaf kind with the hoisted sin / cos on it: (B,R,C), (B,1,C), (1,1,C), (C,), (B,R,1), (1,R,1), (B,1,1), one element
    seed = nd.broadcast_to(nd.asarray(np.float32(0.5)), (2, 3, 8))
    kinds = [x, g, f(1, 1, 8), f(8), f(2, 3, 1), h, f(2, 1, 1), seed]
    for half in (0, 4):                                 # (four kinds per program: the lazy layer cuts a chain at 44 instructions)
        acc = None
        for leaf in kinds[half:half + 4]:
            leaf = nd.broadcast_to(leaf, (2, 3, 8))     # (sin of a smaller pending array would be evaluated first and become the leaf)
            t = nd.multiply(nd.sin(leaf), nd.cos(leaf))
            acc = t if acc is None else nd.add(acc, t)
        arrs.append((f"leaf kinds {half}..", acc))
    acc = kinds[0]
    for leaf in kinds[1:7] + [y]:
        acc = nd.add(nd.multiply(acc, 0.5), leaf)
    arrs.append(("8 leaves", acc))
    out = []
    for name, arr in arrs:
        assert arr._expr is not None and arr.shape == (2, 3, 8), name
        prog, keep = lz.build_program(arr._expr, arr.shape)
        out.append((name, prog, keep))
    return out


def test_batched_kernels_compile(lib, on_gpu, product):
    """Probe kinds 8 (batched strips) and 9 (batched tiled): every unary and binary operator, where, a float64 program with an int64
    leaf, every leaf kind with hoisted sin / cos, 8 leaves and each reduce op compile for gfx950. (The kinds are new: on the parent
    commit they are a ValueError.)"""
    from minidiff_amd import ndarray as nd
    plib, log = product
    prev = nd.set_lazy(True)
    try:
        progs = _probe_programs(nd)
    finally:
        nd.set_lazy(prev)
    assert [p[1].n_leaves for p in progs if p[0].startswith("leaf kinds") or p[0] == "8 leaves"] == [4, 4, 8]
    for name, prog, keep in progs:
        for kind, tag in KINDS.items():
            rops = CODES.values() if name == "leaf kinds 4.." else (_capi.R_SUM,)
            for rop in rops:
                plib.vm_jit_probe(prog, kind, rop, 0, log, len(log))
                assert log.value.startswith(tag), (name, kind, log.value[:40])     # the log of a probe starts with the kernel's name
    with pytest.raises(ValueError):
        plib.vm_jit_probe(progs[0][1], 10, 0, 0, log, len(log))


# ------------------------------------------------------------------------------------------------------------------------ GPU: exact
# (outer, n_red, inner): every value of outer {2, 3, 5}, n_red {1, 2, 63, 67, 511, 512, 515, 1027}, inner {4, 252, 256, 260, 1028};
# the strips form from n_red = 512 on, the tiled one below (generated legs); at most 2.1 M elements
TRIPLES = [(2, 1, 4), (3, 2, 252), (5, 63, 256), (2, 67, 260), (3, 511, 1028), (5, 512, 4), (2, 515, 252), (3, 1027, 256),
           (5, 1, 260), (2, 2, 1028), (3, 63, 4), (5, 67, 252), (2, 511, 256), (3, 512, 260), (2, 1027, 1028), (5, 515, 256),
           (3, 512, 1028), (5, 1027, 4), (2, 63, 1028), (3, 515, 260)]
FORCED_NB = (1, 2, 3, 64)


def _positions(n_red, nb, ru):
    """row 0, the last row, and both sides of every boundary along n_red: the wave interleave (4 lane rows / waves), the band step
    (NB, 4 NB), the RU trip (4 NB RU rows), the pair of trips in flight (twice that), where the tail loop of single rows begins
    (strips: the last whole trip of wave 0; tiled: the last whole pair of rows), and the tiled form's pair (8)"""
    trip = 4 * nb * ru
    pos = {0, n_red - 1}
    for b in (4, 8, nb, 4 * nb, trip, 2 * trip, (n_red // trip) * trip, (n_red // (2 * trip)) * 2 * trip, (n_red // 8) * 8, (n_red // 4) * 4):
        if 0 < b < n_red:
            pos |= {b - 1, b}
    return sorted(pos)


def _columns(inner):
    """the first and the last vector of a strip, both sides of a strip edge (255 | 256), the last vector"""
    return sorted({c for c in (0, 3, 252, 255, 256, 259, inner - 4, inner - 1) if 0 <= c < inner})


@gpu
@pytest.mark.parametrize("outer, n_red, inner", TRIPLES)
def test_exact_gpu(lazy_nd, lib, on_gpu, generated, mdopt, outer, n_red, inner):
    nd = lazy_nd
    assert on_gpu
    shape = (outer, n_red, inner)
    idx = TRIPLES.index(shape)
    form = _form(n_red, generated)
    rng = np.random.default_rng(idx)
    forced = FORCED_NB if form == "strips" else (0,)
    for dt in (f32, f64):
        ru = _ru([dt.itemsize] * 2)
        what = f"{shape} {dt.name} {form}"
        # sum of x * y, small integers: every partial sum is exact in float32 (|sum| <= 16 * 1027 < 2^24)
        x = rng.integers(-4, 5, shape).astype(dt)
        y = rng.integers(-4, 5, shape).astype(dt)
        dx, dy = nd.asarray(x), nd.asarray(y)
        make = lambda: nd.multiply(dx, dy)              # noqa: E731
        ref = _eager(nd, make).sum(axis=1, dtype=np.float64).astype(dt)
        for nb in forced:
            mdopt("sweep_nb", nb)
            _same(_fused(nd, lib, generated, make, "sum", what=what), ref, f"{what}: sum, sweep_nb {nb}")
        mdopt("sweep_nb", 0)
        _same(_fused(nd, lib, generated, make, "sum", keepdims=True, what=what), ref.reshape(outer, 1, inner), f"{what}: sum, keepdims")
        # .. one element changed: exactly one output of one batch changes
        b, r, c = outer // 2, n_red - 1 - (n_red > 3) * 2, inner - 3
        dx[b:b + 1, r:r + 1, c:c + 1] = float(x[b, r, c] + 7)
        exp = ref.copy()
        exp[b, c] += 7 * y[b, r, c]
        _same(_fused(nd, lib, generated, make, "sum", what=what), exp, f"{what}: sum, one element changed")
        # prod of +-2^k factors: signs in x; y holds a run of twos and halves somewhere along n_red in every column, ones elsewhere —
        # any partial product stays within 2^+-12
        x = rng.choice(np.array([-1.0, 1.0]), shape).astype(dt)
        y = np.ones(shape, dt)
        n2, nh = min(12, n_red // 2), min(5, n_red // 4)
        start = rng.integers(0, n_red, (outer, 1, inner))
        for k in range(n2 + nh):
            np.put_along_axis(y, (start + k) % n_red, 2.0 if k < n2 else 0.5, axis=1)
        dx, dy = nd.asarray(x), nd.asarray(y)
        ref = np.prod(_eager(nd, make).astype(np.float64), axis=1).astype(dt)
        assert np.all(np.abs(ref) == 2.0 ** (n2 - nh))
        for nb in forced:
            mdopt("sweep_nb", nb)
            _same(_fused(nd, lib, generated, make, "prod", what=what), ref, f"{what}: prod, sweep_nb {nb}")
        # max / min of twice a permutation, then an extreme or a NaN planted: one run per position, the batch and the column cycling
        x = (rng.permutation(outer * n_red * inner).reshape(shape) - outer * n_red * inner // 2).astype(dt)   # (exact: < 2^23)
        y = np.full(shape, 2.0, dt)
        dx, dy = nd.asarray(x), nd.asarray(y)
        v = _eager(nd, make)
        base = {"max": v.max(axis=1), "min": v.min(axis=1)}
        for nb in forced:
            mdopt("sweep_nb", nb)
            for op in ("max", "min"):
                _same(_fused(nd, lib, generated, make, op, what=what), base[op], f"{what}: {op}, permutation, sweep_nb {nb}")
        nb_req = forced[idx % len(forced)]
        mdopt("sweep_nb", nb_req)
        nb = _nb(outer, n_red, inner, ru, nb_req) if form == "strips" else 1
        big = float(2 ** 25)
        batches, cols = sorted({0, outer // 2, outer - 1}), _columns(inner)
        for i, r in enumerate(_positions(n_red, nb, ru)):
            for b in batches:
                c = cols[(i + b) % len(cols)]
                for op, plant in (("max", big), ("min", -big), ("max", np.nan), ("min", np.nan)):
                    dx[b:b + 1, r:r + 1, c:c + 1] = plant
                    exp = base[op].copy()
                    exp[b, c] = dt.type(plant) * dt.type(2.0)
                    _same(_fused(nd, lib, generated, make, op, what=what), exp, f"{what}: {op}, {plant} planted at ({b}, {r}, {c}), NB {nb}")
                dx[b:b + 1, r:r + 1, c:c + 1] = float(x[b, r, c])
        for op in ("max", "min"):                        # (everything was put back)
            _same(_fused(nd, lib, generated, make, op, what=what), base[op], f"{what}: {op}, restored")
        mdopt("sweep_nb", 0)


# ------------------------------------------------------------------------------------------------- GPU: pinned to the accepted kernels
@gpu
@pytest.mark.parametrize("shape", [(3, 512, 260), (2, 1027, 1028), (5, 515, 256)])
def test_batches_match_the_2d_strips_kernel_gpu(lazy_nd, lib, on_gpu, mdopt, shape):
    """With sweep_nb forced to the same value in both calls, each batch's outputs on random floats have the bits of the existing 2-D
    fused column call on that batch's slice (the strips kernel, jit_min = 1): the batch only moves the bases."""
    nd = lazy_nd
    assert on_gpu
    mdopt("jit", 1)
    mdopt("jit_min", 1)
    outer, n_red, inner = shape
    rng = np.random.default_rng(5)
    for dt in (f32, f64):
        x, y, g = (nd.asarray(rng.standard_normal(s).astype(dt)) for s in (shape, shape, (outer, 1, inner)))
        for nb in FORCED_NB:
            mdopt("sweep_nb", nb)
            s0 = nd.FUSION_STATS["vm_reduce_axis"]
            got = nd.sum(nd.multiply(nd.multiply(x, y), g), axis=1).get()
            assert nd.FUSION_STATS["vm_reduce_axis"] - s0 == 1
            for b in range(outer):
                s0, l0 = nd.FUSION_STATS["vm_reduce"], _launched(lib)
                ref = nd.sum(nd.multiply(nd.multiply(x[b], y[b]), g[b]), axis=0).get()
                assert nd.FUSION_STATS["vm_reduce"] - s0 == 1 and _launched(lib) - l0 == 1
                _same(got[b], ref, f"{shape} {dt.name} sweep_nb {nb}, batch {b}")


@gpu
@pytest.mark.parametrize("shape", [(4, 130, 260), (3, 50, 256), (2, 300, 516)])
def test_leading_axes_match_the_2d_chain_gpu(lazy_nd, lib, on_gpu, generated, shape):
    """sum / max over (0, 1) of a 3-D chain is the 2-D column problem (B R, C): the bits of the same chain over the leaves reshaped
    to 2-D, through the strips kernel (n_red >= 512) and the tiled kernels with their second pass."""
    nd = lazy_nd
    assert on_gpu
    B, R, Cn = shape
    rng = np.random.default_rng(6)
    for dt in (f32, f64):
        xh, rh, wh = (rng.standard_normal(s).astype(dt) for s in (shape, (B, R, 1), (Cn,)))
        x, r, w = nd.asarray(xh), nd.asarray(rh), nd.asarray(wh)
        x2, r2 = nd.asarray(xh.reshape(B * R, Cn)), nd.asarray(rh.reshape(B * R, 1))
        make = lambda: nd.add(nd.multiply(nd.multiply(x, r), w), 0.5)          # noqa: E731
        for op in ("sum", "max"):
            s0 = nd.FUSION_STATS["vm_reduce"]
            ref = getattr(nd, op)(nd.add(nd.multiply(nd.multiply(x2, r2), w), 0.5), axis=0).get()
            assert nd.FUSION_STATS["vm_reduce"] - s0 == 1
            _same(_fused(nd, lib, generated, make, op, (0, 1), what=f"{shape} {op}"), ref, f"{shape} {dt.name} {op} over (0, 1)")
            _same(_fused(nd, lib, generated, make, op, (0, 1), True, f"{shape} {op}"), ref.reshape(1, 1, Cn), f"{shape} {dt.name} {op}, keepdims")
    # a (B,1,C) leaf does not collapse over (B, R): refused, today's value
    g = nd.asarray(rng.standard_normal((B, 1, Cn)).astype(np.float32))
    xs = nd.asarray(rng.standard_normal(shape).astype(np.float32))
    make = lambda: nd.multiply(xs, g)                   # noqa: E731
    v = _eager(nd, make)
    _same(_fallback(nd, make, "max", (0, 1), what="(B,1,C) under (0, 1)"), v.max(axis=(0, 1)), "(B,1,C) under (0, 1)")


# ------------------------------------------------------------------------------------------------------------------- GPU: inexact sums
@gpu
@pytest.mark.parametrize("shape", [(3, 67, 260), (2, 511, 256), (3, 512, 260), (2, 1027, 1028), (5, 515, 256)])
def test_inexact_sums_gpu(lazy_nd, lib, on_gpu, generated, mdopt, shape):
    nd = lazy_nd
    assert on_gpu
    outer, n_red, inner = shape
    form = _form(n_red, generated)
    for dt in (f32, f64):
        rng = np.random.default_rng(n_red)
        x, y = nd.asarray(rng.standard_normal(shape).astype(dt)), nd.asarray(rng.standard_normal(shape).astype(dt))
        make = lambda: nd.multiply(x, y)                # noqa: E731
        v = _eager(nd, make)
        for req in ((0,) + FORCED_NB if form == "strips" else (0,)):
            mdopt("sweep_nb", req)
            nb = _nb(outer, n_red, inner, _ru([dt.itemsize] * 2), req) if form == "strips" else 1
            what = f"{shape} {dt.name} {form} sweep_nb {req}"
            _check_sum(_fused(nd, lib, generated, make, "sum", what=what), v, 1, form, nb, what)


# ------------------------------------------------------------------------------------------------------------------- GPU: leaf kinds
def _leaf_case(nd, name, dt, rng, shape):
    """-> (make, vec): the chain and the item sizes of its unit-stride, row-varying leaves (what RU is chosen from)"""
    B, R, Cn = shape
    f = lambda *s: nd.asarray(rng.standard_normal(s).astype(dt))      # noqa: E731
    x = f(B, R, Cn)
    one = {"dense (B,R,C)": (B, R, Cn), "(B,1,C)": (B, 1, Cn), "(1,1,C)": (1, 1, Cn), "(C,)": (Cn,), "(B,R,1)": (B, R, 1),
           "(1,R,1)": (1, R, 1), "(B,1,1)": (B, 1, 1)}
    if name in one:
        y = f(*one[name])
        return (lambda: nd.multiply(x, y)), [dt.itemsize] * (2 if name == "dense (B,R,C)" else 1)
    if name == "one element, stride 0":
        s = nd.broadcast_to(nd.asarray(dt.type(0.375)), shape)
        return (lambda: nd.add(nd.multiply(x, s), 1.5)), [dt.itemsize]
    if name == "batches with a gap":                                  # a sliced view: the batch stride is not R C
        xs, y = f(B + 1, R + 6, Cn)[1:, :R], f(B, R, Cn)
        return (lambda: nd.multiply(xs, y)), [dt.itemsize] * 2
    if name == "bool under where":
        m = nd.asarray(rng.integers(0, 2, (B, 1, Cn)).astype(bool))
        k = nd.asarray(rng.integers(0, 2, shape).astype(bool))
        return (lambda: nd.where(m, nd.where(k, x, 0.25), nd.negative(x))), [dt.itemsize, 1]
    if name == "all kinds in one chain":
        ys = [f(*s) for s in one.values()]

        def make():
            acc = x
            for y in ys:
                acc = nd.add(nd.multiply(acc, 0.5), y)
            return acc
        return make, [dt.itemsize] * 2
    raise KeyError(name)


LEAF_KINDS = ["dense (B,R,C)", "(B,1,C)", "(1,1,C)", "(C,)", "(B,R,1)", "(1,R,1)", "(B,1,1)", "one element, stride 0",
              "batches with a gap", "bool under where", "all kinds in one chain"]


@gpu
@pytest.mark.parametrize("kind", LEAF_KINDS)
def test_leaf_kinds_gpu(lazy_nd, lib, on_gpu, generated, kind):
    """Every leaf kind the form reads, alone and combined, below and above the strips form's floor: max / min bit for bit, sums
    within the chain-length bound."""
    nd = lazy_nd
    assert on_gpu
    for shape in ((3, 67, 256), (3, 515, 260)):
        form = _form(shape[1], generated)
        for dt in (f32, f64):
            make, vec = _leaf_case(nd, kind, dt, np.random.default_rng(sum(map(ord, kind))), shape)
            nb = _nb(shape[0], shape[1], shape[2], _ru(vec)) if form == "strips" else 1
            what = f"{kind}, {shape}, {dt.name}, {form}"
            v = _eager(nd, make)
            for keepdims in (False, True):
                _check_sum(_fused(nd, lib, generated, make, "sum", 1, keepdims, what), v, 1, form, nb, f"{what}: sum")
            _same(_fused(nd, lib, generated, make, "max", 1, what=what), v.max(axis=1), f"{what}: max")
            _same(_fused(nd, lib, generated, make, "min", 1, True, what), v.min(axis=1, keepdims=True), f"{what}: min, keepdims")


# -------------------------------------------------------------------------------------------------------- GPU: refusals, tickets
@gpu
def test_refusals_fall_back_gpu(lazy_nd, lib, on_gpu, generated):
    nd = lazy_nd
    assert on_gpu
    rng = np.random.default_rng(7)
    f = lambda *s: nd.asarray(rng.standard_normal(s).astype(np.float32))          # noqa: E731
    x = f(3, 64, 256)
    yt = nd.swapaxes(f(3, 256, 64), 1, 2)
    wide = f(3, 64, 264)
    cases = [("a transposed leaf", lambda: nd.multiply(x, yt)),
             ("an unaligned leaf", lambda: nd.multiply(x, wide[:, :, 1:257]))]
    for what, make in cases:
        v = _eager(nd, make)
        got = _fallback(nd, make, "sum", 1, what=what)
        ref = v.sum(axis=1, dtype=np.float64)
        assert np.abs(got - ref).max() <= 34 * 2.0 ** -24 * np.abs(v).sum(axis=1, dtype=np.float64).max(), what
        _same(_fallback(nd, make, "max", 1, what=what), v.max(axis=1), f"{what}: max")
    # two reduced axes of a leaf that do not collapse to one stride: rows 0 .. 7 of 10 under (B, 8, 8, C) reduced over (1, 2)
    x4, y4 = f(3, 8, 8, 256), f(3, 8, 10, 256)[:, :, :8]
    make = lambda: nd.multiply(x4, y4)                  # noqa: E731
    _same(_fallback(nd, make, "max", (1, 2), what="a gap inside the reduced run"), _eager(nd, make).max(axis=(1, 2)), "a gap inside the reduced run")
    # .. while a gap between the batches is the batch stride
    xg = f(4, 70, 256)[:3, :64]
    make = lambda: nd.multiply(xg, x)                   # noqa: E731
    _same(_fused(nd, lib, generated, make, "max", 1, what="a gap between batches"), _eager(nd, make).max(axis=1), "a gap between batches")


@gpu
def test_tickets_gpu(lazy_nd, lib, on_gpu, generated, mdopt):
    """(1025, 512, 4) would need NS outer MD_TICKET_PAD = 16400 > 16384 ticket words for its bands: it runs in one band whatever is
    forced, and is right. Three interleaved repeats of two strips cases give the same bits (the order of combination is the geometry's), and
    afterwards an eager column sum that uses the tickets is still right: the counters are back at zero."""
    nd = lazy_nd
    assert on_gpu
    rng = np.random.default_rng(11)
    shape = (1025, 512, 4)
    assert -(-shape[2] // 256) * shape[0] * TICKET_PAD > TICKET_WORDS
    x, y = rng.integers(-4, 5, shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    dx, dy, dz = nd.asarray(x), nd.asarray(y), nd.asarray(x)
    ints = lambda: nd.multiply(dx, dz)                  # noqa: E731
    _same(_fused(nd, lib, generated, ints, "sum"), (x.astype(np.float64) ** 2).sum(axis=1).astype(np.float32), "(1025, 512, 4): sum of squares")
    flt = lambda: nd.multiply(dx, dy)                   # noqa: E731
    mdopt("sweep_nb", 1)
    one_band = _fused(nd, lib, generated, flt, "sum")
    for nb in (2, 64, 0):
        mdopt("sweep_nb", nb)
        _same(_fused(nd, lib, generated, flt, "sum"), one_band, f"(1025, 512, 4): sweep_nb {nb} against one band")
    makes = []
    for shp in ((3, 1027, 256), (5, 515, 260)):
        a, b = nd.asarray(rng.standard_normal(shp).astype(np.float32)), nd.asarray(rng.standard_normal(shp).astype(np.float32))
        makes.append(lambda a=a, b=b: nd.multiply(nd.exp(a), b))
    first = [_fused(nd, lib, generated, m, "sum") for m in makes]
    for _ in range(2):
        for m, ref in zip(makes, first):
            _same(_fused(nd, lib, generated, m, "sum"), ref, "repeat")
    h = rng.standard_normal((2048, 1024)).astype(np.float32)
    prev = nd.set_lazy(False)
    try:
        got = nd.sum(nd.asarray(h), axis=0).get()
    finally:
        nd.set_lazy(prev)
    ref = h.sum(axis=0, dtype=np.float64)
    assert np.abs(got - ref).max() <= 34 * 2.0 ** -24 * np.abs(h).sum(axis=0, dtype=np.float64).max()


# ----------------------------------------------------------------------------------------------------------------- GPU: end to end
@gpu
def test_scale_and_layer_norm_gradients_gpu(lazy_nd, lib, on_gpu, generated):
    """Through the tape, lazy against eager: d/dg sum((x g)^2) with g of shape (B,1,C) — unbroadcast issues
    sum(.., axis=1, keepdims=True) on the pending product — and d/dgamma, d/dbeta of ((x - mu) r) gamma + beta on a 3-D input with
    gamma, beta of shape (C,): sum(.., axis=(0, 1))."""
    nd = lazy_nd
    assert on_gpu
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    md = build_engine(HipBackendTable, "lazy")
    B, R, Cn = 4, 64, 256

    def scale(dt):
        rng = np.random.default_rng(3)
        X = md.Tensor(rng.standard_normal((B, R, Cn)).astype(dt))
        G = md.Tensor(rng.standard_normal((B, 1, Cn)).astype(dt), allow_grad=True)
        md.sum((X * G) ** 2).backward()
        return [G.grad.as_numpy().astype(np.float64)]

    def layer_norm(dt):
        rng = np.random.default_rng(4)
        x = rng.standard_normal((B, R, Cn)).astype(dt)
        X, MU = md.Tensor(x), md.Tensor(x.mean(axis=-1, keepdims=True).astype(dt))
        RS = md.Tensor((1 / x.std(axis=-1, keepdims=True)).astype(dt))
        GA = md.Tensor(rng.standard_normal(Cn).astype(dt), allow_grad=True)
        BE = md.Tensor(rng.standard_normal(Cn).astype(dt), allow_grad=True)
        md.sum((((X - MU) * RS) * GA + BE) ** 2).backward()
        return [GA.grad.as_numpy().astype(np.float64), BE.grad.as_numpy().astype(np.float64)]

    for sweep, shapes in ((scale, [(B, 1, Cn)]), (layer_norm, [(Cn,), (Cn,)])):
        for dt, tol in ((f32, 1e-6), (f64, 1e-13)):
            nd.set_lazy(False)
            eager = sweep(dt)
            nd.set_lazy(True)
            s0 = nd.FUSION_STATS["vm_reduce_axis"]
            lazy = sweep(dt)
            assert nd.FUSION_STATS["vm_reduce_axis"] - s0 >= 1, sweep.__name__
            for g_l, g_e, shp in zip(lazy, eager, shapes):
                assert g_l.shape == shp
                assert np.linalg.norm(g_l - g_e) <= tol * np.linalg.norm(g_e), (sweep.__name__, dt, np.linalg.norm(g_l - g_e) / np.linalg.norm(g_e))
