"""std and argmax / argmin over a MIDDLE axis of a C-contiguous array: (outer, n, inner) as `outer` independent column problems in
one launch (csrc/moments.hip: the batched column form of mdhip_var; csrc/reduce.hip: the batched launch of k_arg_cols_strips).
Which forms take the kernels, that they agree with NumPy (std within the bounds of test_std_fused.py, the arg functions bit for
bit: first occurrence, first NaN), that batches do not read each other's partial rows / ticket words / sums, that options
var_batched / arg_batched switch the new forms off, and that every other middle-axis form is composed as before. The shapes are
the smallest that reach every branch of the two launchers; the reduced axis is the second member of each entry."""
import ctypes as C
import functools

import numpy as np
import pytest

from minidiff_amd import ndarray as nd

# (shape, reduced axis): what each reaches
SHAPES = [
    ((2, 64, 256), 1),        # every minimum at once
    ((3, 67, 260), 1),        # a ragged last strip (clamped lanes), a row tail that is no multiple of the batch depth
    ((5, 200, 512), 1),       # NB > 1: band partials, tickets, several batches sharing the ticket block
    ((300, 64, 256), 1),      # more strips x batches than CUs: NB == 1
    ((2, 3, 64, 256), 2),     # two leading axes collapse into `outer`
    ((2, 64, 4, 64), 1),      # trailing axes collapse into inner = 256
    ((1, 128, 512), 1),       # outer == 1 on a 3-D array
]
FLOATS = [np.float32, np.float64]


def _tol(dtype):      # the bounds of test_std_fused.py for this kernel family
    return 8 * (2e-6 if dtype == np.float32 else 1e-13)


def _view3(shape, axis):
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    return outer, shape[axis], inner


@functools.lru_cache(maxsize=None)
def _std_case(shape, dtype):
    """The host array of a table entry — drawn once, shared between the tests, read-only."""
    seed = 61 + sum(shape)
    h = (np.random.default_rng(seed).standard_normal(shape) * 3 + 10).astype(dtype)     # the data of test_std_fused.py: a mean far from 0
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def _std_ref(shape, axis, dtype, ddof):
    r = np.std(_std_case(shape, dtype).astype(np.float64), axis=axis, ddof=ddof, keepdims=True).astype(dtype)
    r.setflags(write=False)
    return r


@pytest.fixture
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


# ---- 1. std takes the kernel and matches NumPy --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
def test_std_over_a_middle_axis_takes_the_kernel_and_matches_numpy(lib, on_gpu, eager, dtype):
    assert on_gpu
    for shape, axis in SHAPES:
        h = _std_case(shape, dtype)
        d = nd.asarray(h)
        for ddof in (0, 1):
            ref = _std_ref(shape, axis, dtype, ddof)
            for keep in (False, True):
                fused = nd._std_fused(d, axis, None, ddof, keep, shape[axis])
                assert fused is not None, (shape, axis, ddof, keep)
                exp = ref if keep else ref.reshape(shape[:axis] + shape[axis + 1:])
                assert fused.shape == exp.shape and fused.dtype == exp.dtype, (shape, keep)
                np.testing.assert_allclose(fused.get(), exp, rtol=_tol(dtype), atol=0, err_msg=str((shape, ddof, keep)))
                got = nd.std(d, axis=axis, ddof=ddof, keepdims=keep)
                assert got.shape == exp.shape and got.dtype == exp.dtype
                np.testing.assert_array_equal(got.get(), fused.get())


# ---- 2. batches do not leak into each other ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("outer,n,inner", [(5, 200, 512), (300, 64, 256)])
def test_std_batches_do_not_leak_into_each_other(lib, on_gpu, eager, dtype, outer, n, inner):
    assert on_gpu
    slab = (np.random.default_rng(62).standard_normal((n, inner)) * 3 + 10).astype(dtype)
    h = np.ascontiguousarray(np.broadcast_to(slab, (outer, n, inner)))
    d = nd.asarray(h)
    assert nd._std_fused(d, 1, None, 0, False, n) is not None
    first = nd.std(d, axis=1).get()
    assert np.array_equal(nd.std(d, axis=1).get(), first)                     # bit-identical from call to call
    for b in range(outer):
        assert np.array_equal(first[b], first[0]), b                          # the same slab -> the same bits in every batch
    h[2, n // 2, 7] = 1e6
    got = nd.std(nd.asarray(h), axis=1).get()
    changed = np.argwhere(got != first)
    assert changed.tolist() == [[2, 7]], changed[:8]                          # one column of batch 2, nothing else
    np.testing.assert_allclose(got[2, 7], np.std(h[2, :, 7].astype(np.float64)), rtol=_tol(dtype))


# ---- 3. A/B by option ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", FLOATS)
def test_option_var_batched_switches_the_kernel_off_and_on(lib, on_gpu, eager, mdopt, dtype):
    assert on_gpu
    for shape, axis in SHAPES:
        outer, n, _ = _view3(shape, axis)
        h = _std_case(shape, dtype)
        d = nd.asarray(h)
        fused = nd._std_fused(d, axis, None, 0, False, n)
        assert fused is not None, shape
        mdopt("var_batched", 0)
        assert nd._std_fused(d, axis, None, 0, False, n) is None, shape
        composed = nd.std(d, axis=axis)
        np.testing.assert_allclose(composed.get(), np.std(h, axis=axis), rtol=2e-5)     # the composition's bound (test_std_fused.py)
        mdopt("var_batched", 1)
        again = nd._std_fused(d, axis, None, 0, False, n)
        assert again is not None and np.array_equal(again.get(), fused.get()), shape


def test_the_option_table_knows_var_batched_and_arg_batched(lib):
    for name in ("var_batched", "arg_batched"):
        v = C.c_int64(-7)
        lib.debug_get_option(name.encode(), C.byref(v))
        assert v.value == 1, name


# ---- 4. forms that stay composed -------------------------------------------------------------------------------------------------
def _check_other_forms_stay_composed(on_gpu):
    rng = np.random.default_rng(63)
    prev = nd.set_lazy(False)
    try:
        def normal(shape, dtype):
            return (rng.standard_normal(shape) * 3 + 10).astype(dtype)

        cases = [                                                              # (array, axis, dtype=)
            (nd.asarray(normal((4, 63, 256), np.float32)), 1, None),           # one row short
            (nd.asarray(normal((4, 64, 252), np.float32)), 1, None),           # under 256 columns
            (nd.asarray(normal((4, 64, 258), np.float32)), 1, None),           # not a whole 16-B vector
            (nd.asarray(normal((4, 64, 256), np.float32))[:, :, ::2], 1, None),    # not contiguous
            (nd.asarray(normal((4, 64, 256), np.float32)), 1, np.float64),     # a different accumulation dtype
            (nd.asarray(rng.integers(-50, 50, (4, 64, 256)).astype(np.int32)), 1, None),   # integers: NumPy answers in float64
        ]
        if not on_gpu:      # the CPU double refuses a middle axis between two extents > 1: a CPU session composes exactly as before
                            # ((1,[128],512) is left out: a unit leading extent makes it the 2-D column form, which the double serves)
            cases += [(nd.asarray(_std_case(shape, dt)), axis, None) for shape, axis in SHAPES[:-1] for dt in FLOATS]
        nd.set_lazy(True)
        pending = nd.asarray(normal((4, 64, 256), np.float32)) * 2             # a pending lazy expression
        nd.set_lazy(False)
        cases.append((pending, 1, None))
        for arr, axis, dt in cases:
            assert nd._std_fused(arr, axis, dt, 0, False, arr.shape[axis]) is None, (arr.shape, arr.dtype, dt)
            got = nd.std(arr, axis=axis, dtype=dt)
            exp = np.std(arr.get(), axis=axis, dtype=dt)
            assert got.dtype == exp.dtype and got.shape == exp.shape
            np.testing.assert_allclose(got.get(), exp, rtol=2e-5 if exp.dtype == np.float32 else 1e-12)
    finally:
        nd.set_lazy(prev)


def test_other_middle_axis_forms_stay_composed(lib, on_gpu):      # on whichever library the session is bound to
    _check_other_forms_stay_composed(on_gpu)


@pytest.mark.gpu
def test_other_middle_axis_forms_stay_composed_gpu(lib, on_gpu):  # the floors mdhip_var now judges alone, on the product library
    assert on_gpu and lib.target == "hip:gfx950"
    _check_other_forms_stay_composed(True)


# ---- 5. argmax / argmin bit for bit -----------------------------------------------------------------------------------------------
_ARG = (("argmax", nd.argmax, np.argmax), ("argmin", nd.argmin, np.argmin))


ARG_DTYPES = [np.float32, np.float64, np.int32, np.int64]


def _check_arg_over_a_middle_axis(mdopt, dtype):
    rng = np.random.default_rng(64)
    for shape, axis in SHAPES:
        outer, n, inner = _view3(shape, axis)
        h = rng.integers(0, 8, shape).astype(dtype)                            # eight distinct values: every column has ties
        d = nd.asarray(h)
        base = {}
        for name, dev_fn, np_fn in _ARG:
            for keep in (False, True):
                got = dev_fn(d, axis=axis, keepdims=keep)
                assert got.dtype == np.int64
                exp = np_fn(h, axis=axis, keepdims=keep)
                assert got.shape == exp.shape
                assert np.array_equal(got.get(), exp), (name, shape, keep)
            base[name] = np_fn(h, axis=axis).reshape(outer, inner)

        variants = [("ties", h)]
        if np.dtype(dtype).kind == "f":
            # the first NaN wins: three NaNs in a few columns — the FIRST in row 11 (a late band of (5,[200],512): band 11 % 6 = 5),
            # later ones in the middle and in the last row (earlier bands) — and columns whose only NaN is in the last row
            hn = h.copy()
            v = hn.reshape(outer, n, inner)
            for b, c in ((0, 0), (outer - 1, inner - 1), (outer // 2, 257 % inner), (outer - 1, 3)):
                v[b, [11, n // 2, n - 1], c] = np.nan
            for b, c in ((0, 5), (outer - 1, inner - 2)):
                v[b, n - 1, c] = np.nan
            for name, dev_fn, np_fn in _ARG:
                exp = np_fn(hn, axis=axis)
                assert exp.reshape(outer, inner)[0, 0] == 11 and exp.reshape(outer, inner)[0, 5] == n - 1
                assert np.array_equal(dev_fn(nd.asarray(hn), axis=axis).get(), exp), (name, shape, "nan")
            variants.append(("nan", hn))

        # a unique extreme in the last / the first row of every column of ONE batch: that row there, the other batches unchanged
        b = min(2, outer - 1)
        for row in (n - 1, 0):
            for name, dev_fn, np_fn in _ARG:
                hx = h.copy()
                hx.reshape(outer, n, inner)[b, row, :] = 100 if name == "argmax" else -100
                got = dev_fn(nd.asarray(hx), axis=axis).get().reshape(outer, inner)
                assert (got[b] == row).all(), (name, shape, row)
                keep_rows = np.arange(outer) != b
                assert np.array_equal(got[keep_rows], base[name][keep_rows]), (name, shape, row)

        # option parity: the fallback kernels and the batched strips kernel agree bit for bit
        mdopt("arg_batched", 0)
        for tag, hv in variants:
            dv = nd.asarray(hv)
            for name, dev_fn, np_fn in _ARG:
                assert np.array_equal(dev_fn(dv, axis=axis).get(), np_fn(hv, axis=axis)), (name, shape, tag, "arg_batched=0")
        mdopt("arg_batched", 1)


@pytest.mark.parametrize("dtype", ARG_DTYPES)
def test_argmax_argmin_over_a_middle_axis_are_numpys(lib, eager, mdopt, dtype):      # the double: the generic loop
    _check_arg_over_a_middle_axis(mdopt, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ARG_DTYPES)
def test_argmax_argmin_over_a_middle_axis_are_numpys_gpu(lib, on_gpu, eager, mdopt, dtype):   # the batched k_arg_cols_strips launch
    assert on_gpu and lib.target == "hip:gfx950"
    _check_arg_over_a_middle_axis(mdopt, dtype)


# ---- 6. tape level ----------------------------------------------------------------------------------------------------------------
def _run(md, x, graph):
    try:
        t = md.Tensor(x, allow_grad=True)
        y = graph(md, t)
        fwd = y.as_numpy()
    except Exception as e:          # noqa: BLE001 — the reference's own failure for this axis form is what is compared
        return ("raised-forward", type(e))
    try:
        (md.sum(y * y) if graph is _g_std else md.sum(y)).backward()
        return ("ok", fwd, t.grad.as_numpy())
    except Exception as e:          # noqa: BLE001
        return ("raised-backward", type(e), fwd)


def _g_std(md, t):
    return md.std(t, axis=(1,))


def _g_max(md, t):
    return md.max(t, axis=1)


def _check_tape_against_the_oracle(engines, graph):
    """Bounds of test_tape_std_forward_and_backward_against_the_oracle. Where the reference's own graph raises for this axis form
    (reference defects are preserved), the device engine must raise the same way at the same stage."""
    hip, ora = engines
    x = np.random.default_rng(65).standard_normal((3, 64, 256)).astype(np.float64) + 2.0
    dev, ref = _run(hip, x, graph), _run(ora, x, graph)
    assert dev[0] == ref[0], (dev[:2], ref[:2])
    if ref[0] == "ok":
        np.testing.assert_allclose(dev[1], ref[1], rtol=1e-12)
        np.testing.assert_allclose(dev[2], ref[2], rtol=1e-10, atol=1e-13)
    elif ref[0] == "raised-backward":
        assert dev[1] is ref[1], (dev[1], ref[1])
        np.testing.assert_allclose(dev[2], ref[2], rtol=1e-12)
    else:
        assert dev[1] is ref[1], (dev[1], ref[1])


@pytest.mark.parametrize("graph", [_g_std, _g_max], ids=["std", "max"])
def test_tape_middle_axis_against_the_oracle(engines, graph):
    _check_tape_against_the_oracle(engines, graph)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [_g_std, _g_max], ids=["std", "max"])
def test_tape_middle_axis_against_the_oracle_gpu(lib, on_gpu, engines, graph):      # std forward: the batched var kernel; max's vjp: the batched arg kernel
    assert on_gpu and lib.target == "hip:gfx950"
    _check_tape_against_the_oracle(engines, graph)
