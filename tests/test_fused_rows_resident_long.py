"""Lazy mode, MDHIP_LAZY_ROWS with MDHIP_LAZY_ROWS_MAX raised (ndarray.set_lazy_rows_max): rows of 2052 .. 8192 elements in one launch
of the staged program's BLOCK-per-row form, k_fused_rowsresb<G>: 256 lanes per row, G = ceil(n_red / 1024) vector
groups per lane held in registers across the stages, each stage combined in the order of the generated block-per-row reduction.

CPU  the compile-only probe (kind 10) at every G the tests launch and at the register ceiling, the probe's bounds, the setter and its
     default, and — the test double refuses staged programs — that raising the maximum changes no bit and no reduction count there.
GPU  the staged launch against the COMPOSED route (tests/test_fused_rows_resident.py: mdhip_vm_reduce per stage, then mdhip_vm_eval)
     bit for bit on both sides of every G step; against NumPy with operands exact in any order, through every leaf mode; special
     values; launch counts; refusals that compose; the tape. The helpers are those of tests/test_fused_rows_resident.py."""
import ctypes as C

import numpy as np
import pytest

from test_fused_rows_resident import (RED_STATS, _abi_programs, _both, _composed, _exact_cases, _launched, _layer_norm, _raw_program,  # noqa: F401  (fixtures)
                                      _same, _softmax, _staged_padded, _tape_softmax_xent, _words, _workloads, generated, product)

gpu = pytest.mark.gpu
f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
MIN_OUT = 256       # fusion.hip: VM_ROWS_MIN_OUT, the fewest rows a block-per-row launch takes


def _g(n_red):
    """vector groups per lane: the row's 16-byte groups over 256 lanes"""
    return -(-(n_red // 4) // 256)


@pytest.fixture
def long_nd(lib):
    """lazy mode, the rows switch ON and rows up to 8192 recorded; all three put back afterwards"""
    from minidiff_amd import ndarray as nd
    prev, prev_rows, prev_max = nd.set_lazy(True), nd.set_lazy_rows(True), nd.set_lazy_rows_max(8192)
    yield nd
    nd.set_lazy_rows_max(prev_max)
    nd.set_lazy_rows(prev_rows)
    nd.set_lazy(prev)


@pytest.fixture
def remarks(product):
    """the product library with jit_verbose = 2: the compiler's resource remarks in the log of every compilation"""
    plib, log = product
    old = C.c_int64()
    plib.debug_get_option(b"jit_verbose", C.byref(old))
    plib.debug_set_option(b"jit_verbose", 2)
    yield plib, log
    plib.debug_set_option(b"jit_verbose", old.value)


# ------------------------------------------------------------------------------------------------------------- CPU: compile-only
@pytest.mark.parametrize("n_red", [2052, 4096, 5120, 8192])
@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_block_form_compiles_without_scratch(long_nd, remarks, dt, n_red):
    nd = long_nd
    from minidiff_amd import lazy as lz
    plib, log = remarks
    assert _g(n_red) == {2052: 3, 4096: 4, 5120: 5, 8192: 8}[n_red]
    for what, make in _workloads(nd, dt, MIN_OUT, n_red):
        p = make()
        assert p._expr is not None and lz.live_rows(p._expr), what
        prog, keep = lz.build_program(p._expr, p.shape)
        plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
        text = log.value.decode()
        assert text.startswith(f"k_fused_rowsresb{_g(n_red)}_"), (what, text[:80])
        assert "ScratchSize [bytes/lane]: 0" in text, (what, n_red, dt, text)


def _full_leaves(nd, dt, shape, n_leaves, seed=0):
    rng = np.random.default_rng(seed)
    return [nd.asarray(rng.standard_normal(shape).astype(dt)) for _ in range(n_leaves)]


def _full_leaf_layer_norm(nd, ls):
    """a layer norm whose operand (a sum of all but two of the arrays), gamma and beta are all full arrays: len(ls) vector leaves"""
    x = ls[0]
    for leaf in ls[1:-2]:
        x = nd.add(x, leaf)
    return _layer_norm(nd, x, ls[-2], ls[-1])


def test_block_form_compiles_at_the_register_ceiling(long_nd, remarks):
    """VM_STAGED_HELD_MAX = 256 held registers per lane: four float64 vector leaves at G = 8 hold exactly 256 and compile without
    scratch; a fifth is refused, not spilled."""
    nd = long_nd
    from minidiff_amd import lazy as lz
    plib, log = remarks
    for n_leaves, fits in ((4, True), (5, False)):
        p = _full_leaf_layer_norm(nd, _full_leaves(nd, f64, (MIN_OUT, 8192), n_leaves))
        assert len(lz.live_rows(p._expr)) == 2
        prog, keep = lz.build_program(p._expr, p.shape)
        assert prog.n_leaves == n_leaves
        if not fits:
            with pytest.raises(ValueError):
                plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
            continue
        plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
        text = log.value.decode()
        assert text.startswith("k_fused_rowsresb8_") and "ScratchSize [bytes/lane]: 0" in text, text


def test_probe_boundaries(long_nd, product):
    nd = long_nd
    plib, log = product
    for n_red, name in ((2048, "k_fused_rowsres8_"), (2052, "k_fused_rowsresb3_"), (8192, "k_fused_rowsresb8_"), (8196, None)):
        x = nd.asarray(np.zeros((4, n_red), np.float32))
        prog = _raw_program(f32, _words(_abi_programs(n_red)[1][2], n_red), [x], (4, n_red))
        if name is None:
            with pytest.raises(ValueError):
                plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
        else:
            plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
            assert log.value.decode().startswith(name), (n_red, log.value.decode()[:80])


# ------------------------------------------------------------------------------------------------------------------ CPU: the setter
def test_rows_max_setter(lib):
    from minidiff_amd import ndarray as nd
    start = nd.lazy_rows_max()
    try:
        assert nd.set_lazy_rows_max(2048) == start and nd.lazy_rows_max() == 2048
        assert nd.set_lazy_rows_max(8192) == 2048 and nd.lazy_rows_max() == 8192
        assert nd.set_lazy_rows_max(np.int64(4096)) == 8192 and nd.lazy_rows_max() == 4096
        for bad in (2047, 8193, 0, -1, 4096.0, "4096", None, True):
            with pytest.raises(ValueError):
                nd.set_lazy_rows_max(bad)
            assert nd.lazy_rows_max() == 4096, bad
    finally:
        nd.set_lazy_rows_max(start)


def test_rows_max_default_and_environment(lib, monkeypatch):
    """MDHIP_LAZY_ROWS_MAX is read once, when the module is imported: 2048 without it, and a later change of it changes nothing"""
    import os
    from minidiff_amd import ndarray as nd
    assert nd.lazy_rows_max() == int(os.environ.get("MDHIP_LAZY_ROWS_MAX", "2048"))
    monkeypatch.delenv("MDHIP_LAZY_ROWS_MAX", raising=False)
    assert nd._rows_max_from_env() == 2048
    for value, want in (("8192", 8192), ("2052", 2052), ("2048", 2048)):
        monkeypatch.setenv("MDHIP_LAZY_ROWS_MAX", value)
        before = nd.lazy_rows_max()
        assert nd._rows_max_from_env() == want and nd.lazy_rows_max() == before
    for value in ("2047", "8196", "many", "4096.0", ""):
        monkeypatch.setenv("MDHIP_LAZY_ROWS_MAX", value)
        with pytest.raises(ValueError):
            nd._rows_max_from_env()


@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_refused_long_rows_compose_to_the_switch_off_result(long_nd, on_gpu, mdopt, dt):
    """Under the test double every staged program is refused (on a device: with jit 0), so with the maximum raised the long rows are
    recorded, refused and composed: the switch-off bits, the switch-off reduction counts, no staged launch."""
    nd = long_nd
    from minidiff_amd import lazy as lz
    if on_gpu:
        mdopt("jit", 0)
    for n_red in (2052, 4096):
        x = nd.asarray(np.zeros((MIN_OUT, n_red), dt))
        assert nd.max(x, axis=-1, keepdims=True)._expr.kind == lz.ROWRED, "recorded"
        wl = _workloads(nd, dt, MIN_OUT, n_red)
        for what, make in (wl[0], wl[2]):
            off, on, s_off, s_on = _both(nd, make)
            _same(on, off, f"{what} {n_red}")
            assert [s_on[k] for k in RED_STATS] == [s_off[k] for k in RED_STATS], (what, s_off, s_on)
            assert s_on["vm_eval_rows"] == 0 and s_off["vm_eval_rows"] == 0


def test_rows_max_without_the_switch_records_nothing(long_nd):
    nd = long_nd
    nd.set_lazy_rows(False)
    for n_red in (16, 2052, 4096):
        x = nd.asarray(np.zeros((MIN_OUT, n_red), np.float32))
        assert nd.max(x, axis=-1, keepdims=True)._expr is None
    nd.set_lazy_rows(True)
    # and the maximum is the bound: one group more is not recorded, nor are long rows under the floor of 256 rows
    nd.set_lazy_rows_max(4096)
    assert nd.max(nd.asarray(np.zeros((MIN_OUT, 4096), np.float32)), axis=-1, keepdims=True)._expr is not None
    assert nd.max(nd.asarray(np.zeros((MIN_OUT, 4100), np.float32)), axis=-1, keepdims=True)._expr is None
    assert nd.max(nd.asarray(np.zeros((MIN_OUT - 1, 4096), np.float32)), axis=-1, keepdims=True)._expr is None


# =================================================================================================================== GPU
N_RED = [2052, 3072, 3076, 4096, 4100, 5120, 5124, 6144, 6148, 7168, 7172, 8192]     # the first long row, both sides of each G step
N_OUT = [256, 257]


@gpu
@pytest.mark.parametrize("n_red", N_RED)
def test_block_form_equals_the_composed_route_gpu(long_nd, lib, on_gpu, generated, n_red):
    nd = long_nd
    assert on_gpu
    for dt in (f32, f64):
        for n_out in N_OUT:
            rng = np.random.default_rng(n_red * 1000 + n_out)
            x = nd.asarray((rng.standard_normal((n_out, n_red)) * 2).astype(dt))
            gamma, beta = nd.asarray(rng.standard_normal(n_red).astype(dt)), nd.asarray(rng.standard_normal(n_red).astype(dt))
            for what, n_leaves, instrs in _abi_programs(n_red):
                leaves = [x, gamma, beta][:n_leaves]
                shape = (n_out, n_red)
                got = _staged_padded(nd, lib, _raw_program(dt, _words(instrs, n_red), leaves, shape), shape, dt)    # (asserts ONE launch)
                _same(got, _composed(nd, lib, dt, instrs, leaves, shape, n_red), f"{what} {dt.name} {shape}")


@gpu
@pytest.mark.parametrize("shape,axes", [((256, 2052), (1,)), ((2, 128, 4100), (2,)), ((4, 64, 2, 1028), (2, 3))], ids=str)
def test_exact_against_numpy_gpu(long_nd, lib, on_gpu, generated, shape, axes):
    """_exact_cases' integer operands: a row of 8192 sums to less than 2^24 in magnitude, weight and element included up to 4100"""
    nd = long_nd
    assert on_gpu
    from minidiff_amd import lazy as lz
    for dt in (f32, f64):
        for what, make, ref in _exact_cases(nd, dt, shape, axes):
            p = make()
            assert p._expr is not None and lz.live_rows(p._expr), what
            prog, keep = lz.build_program(p._expr, p.shape)
            _same(_staged_padded(nd, lib, prog, shape, dt), ref.astype(dt), f"{what} {dt.name} {shape} (C-ABI)")
            s0 = nd.FUSION_STATS["vm_eval_rows"]
            _same(p.get(), ref.astype(dt), f"{what} {dt.name} {shape}")
            assert nd.FUSION_STATS["vm_eval_rows"] - s0 == 1, what


@gpu
def test_special_values_gpu(long_nd, lib, on_gpu, generated):
    nd = long_nd
    assert on_gpu
    n_red = 2056
    for dt in (f32, f64):
        xh = np.random.default_rng(n_red).standard_normal((MIN_OUT, n_red)).astype(dt)
        xh[1, 3] = np.nan
        xh[2, :] = -np.inf
        xh[3, n_red - 1] = np.inf
        xh[4, 0], xh[4, 1500] = np.nan, np.inf
        xh[5, :] = np.inf
        x = nd.asarray(xh)
        off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, x))
        assert s_on["vm_eval_rows"] == 1 and s_off["vm_eval_rows"] == 0
        _same(on, off, f"softmax {dt.name} {n_red}")
        assert np.isnan(on[1]).all() and np.isnan(on[2]).all() and np.isnan(on[3, n_red - 1]) and np.isnan(on[4]).all() and np.isnan(on[5]).all()
        assert np.isfinite(on[0]).all() and np.isfinite(on[6:]).all()


def _counted(nd, lib, make):
    s0, l0 = dict(nd.FUSION_STATS), _launched(lib)
    v = make().get()
    return v, {k: nd.FUSION_STATS[k] - s0[k] for k in s0}, _launched(lib) - l0


@gpu
@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_launch_counts_gpu(long_nd, lib, on_gpu, generated, dt):
    nd = long_nd
    assert on_gpu
    for what, make in _workloads(nd, dt, MIN_OUT, 4096, seed=5):
        nd.set_lazy_rows(False)
        off, s_off, l_off = _counted(nd, lib, make)
        nd.set_lazy_rows(True)
        nd.set_lazy_rows_max(2048)
        low, s_low, l_low = _counted(nd, lib, make)
        nd.set_lazy_rows_max(8192)
        on, s_on, l_on = _counted(nd, lib, make)
        # 8192: ONE generated launch and nothing else; 2048: exactly the switch-off route
        assert l_on == 1 and s_on["vm_eval_rows"] == 1, (what, l_on, s_on)
        assert s_on["vm_eval"] == 0 and all(s_on[k] == 0 for k in RED_STATS), (what, s_on)
        assert s_low == s_off and l_low == l_off and s_off["vm_eval_rows"] == 0, (what, s_off, s_low)
        _same(low, off, f"{what} {dt.name}, max 2048 against off")
        if what == "layer norm":
            # with the switch off the mean of the CONCRETE x is the eager reduction, whose order is not the fused kernels': held to
            # the bound of tests/test_fused_rows_resident.py::test_launch_counts_gpu (1e-6 / 1e-13 of the norm)
            tol = 1e-6 if dt == f32 else 1e-13
            on64, off64 = on.astype(np.float64), off.astype(np.float64)
            assert np.linalg.norm(on64 - off64) <= tol * np.linalg.norm(off64), (what, dt, np.linalg.norm(on64 - off64) / np.linalg.norm(off64))
        else:
            _same(on, low, f"{what} {dt.name}, max 8192 against max 2048")


@gpu
def test_refusals_compose_gpu(long_nd, lib, on_gpu, generated, mdopt):
    nd = long_nd
    assert on_gpu
    rng = np.random.default_rng(9)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)          # noqa: E731
    # the library's own refusals, asked directly: fewer rows than the floor, and a row one group longer than a block holds
    for shape in ((MIN_OUT - 1, 4096), (MIN_OUT, 8196)):
        xs = nd.asarray(f(*shape))
        prog = _raw_program(f32, _words(_abi_programs(shape[1])[1][2], shape[1]), [xs], shape)
        out = nd.DeviceArray.empty(shape, np.float32)
        with pytest.raises(ValueError):
            lib.vm_eval(prog, out.desc())
        off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, xs))
        assert s_on["vm_eval_rows"] == 0 and s_on == s_off, (shape, s_off, s_on)
        _same(on, off, f"softmax {shape}")
    flat = nd.asarray(f(MIN_OUT * 4096 + 4))
    unaligned = nd.reshape(flat[1:1 + MIN_OUT * 4096], (MIN_OUT, 4096))
    x = nd.asarray(f(MIN_OUT, 4096))
    five = _full_leaves(nd, f64, (MIN_OUT, 8192), 5, seed=10)
    for what, make in (("an unaligned leaf", lambda: _softmax(nd, unaligned)),
                       ("five float64 vector leaves at 8192: over the held-register ceiling", lambda: _full_leaf_layer_norm(nd, five))):
        off, on, s_off, s_on = _both(nd, make)
        assert s_on["vm_eval_rows"] == 0, what
        _same(on, off, what)
    mdopt("jit", 0)
    off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, x))
    assert s_on["vm_eval_rows"] == 0 and s_on == s_off
    _same(on, off, "jit off")


@gpu
@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_softmax_cross_entropy_through_the_tape_gpu(long_nd, lib, on_gpu, generated, dt):
    """(256, 4096) logits, loss and logits' gradient: bit-equal to the switch-off lazy run"""
    nd = long_nd
    assert on_gpu
    off, on, s_off, s_on = _both(nd, lambda: [nd.asarray(a) for a in _tape_softmax_xent(nd, dt, MIN_OUT, 4096)])
    assert s_on["vm_eval_rows"] == 1 and s_off["vm_eval_rows"] == 0, s_on       # the probabilities: max, row sum and chain in one launch
    _same(on[0], off[0], "loss")
    _same(on[1], off[1], "gradient")
    _same(on[2], off[2], "probabilities")
