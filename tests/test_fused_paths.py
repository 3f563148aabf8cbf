"""Every base launch form of lazy mode (csrc/fusion.hip, csrc/fusion_jit.inc) — the (rows, inner) and the generic evaluation, the full
reduction, the tiled and the strips column reduction, the strips form that also stores the evaluated value, the multi-output
evaluation — through the generated kernels AND through the interpreter, bit for bit. (The trailing-axis, middle-axis and three /
four-axis forms have tables of their own: test_fused_rows.py, test_fused_axis.py, test_jit_axes.py.)

The centre is TABLE: what an entry reaches (kernel, generated or interpreter, branch), the shape, the programs, the leaves (each a
view cut from a NaN-filled base), the output views (each inside a sentinel base of this module's own: the WHOLE base is compared, so
a store outside the view fails and an unwritten output fails), the reduce op, the options, and the number of generated launches the
call must make (mdhip_vm_jit_stats; 0 where the form has no generated kernel or the launcher must decline). Every entry runs through
the C-ABI as DeviceArray._materialize and the reducers call it (lazy.build_program + lib.vm_eval / vm_reduce / vm_eval_reduce_cols /
vm_eval_multi), once with jit = 1, jit_min = 1 and once with jit = 0. The `reaches` column is confirmed by a kernel trace of the gpu
half (profiles/README.md: fused_paths_kernel_stats.csv).

Where the numbers come from (MD_BLOCK 256, MD_NUM_CUS 256; a vector group is 4 elements whatever the leaf's storage type; the functions
named are those of fusion.hip's launch planners plan_eval / plan_reduce, which choose the form and its numbers before anything is launched):
  md_grid_for / stream_grid     min(ceil(work / 256), cap) blocks, work = rows * nv + (4 if rows == 1: the tail lanes); the default cap
                                is 2048 (interpreter), 256 * eval_blocks (generated EVAL: 8 / 4 / 2 per CU for <= 2 / 3 / >= 4
                                16-byte streams) or 1024 (RED_ALL). Option max_blocks replaces every one of them: max_blocks = 3
                                makes the grid stride T = 768 groups in both legs (work >= 513).
  k_vm_eval_fast, k_vm_reduce_all  one group per lane and trip (VG = 1), then — 1-D only — lanes 0 .. n % 4 - 1 take the tail.
  EVAL, RED_ALL (U = 2)         main loop while v + (U - 1) * T < total, then the one-group loop. Group counts 767 / 768 (no main
                                trip; last lane idle / busy), 769 (lane 0 alone has a main trip), 1535 / 1536 / 1537 (every lane a
                                main trip; 1537: lane 0 a one-group trip as well), 2305, 3073 (main loop, then the one-group loop).
                                Option jit_u sets U of EVAL (not of RED_ALL): at 3 * 768 + 1 and 4 * 768 + 1 groups U = 1 never
                                enters the one-group loop, U = 3 leaves lane 0 one resp. two such trips behind its main trip, U = 4
                                none (2305: lane 0's four groups are exactly one main trip) resp. one.
  fewer than 4 elements         n = 2, 3: nv = 0, work = 4, one block, the tail lanes alone. n = 1 collapses to ZERO axes
                                (md_vm_build_iter drops extent-1 axes): fast_geometry refuses it, the evaluation runs on
                                k_vm_eval_generic and mdhip_vm_reduce returns "geometry not supported" (the public call then reduces
                                the materialised value): the entries eval-1d-nv0+1 and refuse-reduce-one-element.
  JPos::advance                 (dq, dr) = divmod(T, nv), nv groups per row: inner 20 / 28 (nv 5 / 7: dq and dr non-zero), 3072 (nv
                                768: dr = 0 — rows * 768 groups are whole trips, so this one ends on a full trip), 4000 (nv 1000:
                                dq = 0 and the wrap at cv >= nv). Rows 400 / 331 / 3 / 3: 2000 = 2 T + 464, 2317 = 3 T + 13,
                                2304 = 3 T, 3000 = 3 T + 696 groups. A 2-D program stays 2-D only if some leaf does not collapse:
                                a (C,) leaf, a (R, 1) leaf or a padded row pitch.
  fast_geometry                 one or two collapsed axes; rows > 1 needs inner % 4 == 0; the output unit-stride, dense rows, on its
                                vector alignment min(16, 4 * element size); every leaf inner stride 0 or 1, a unit-stride one
                                aligned and (rows > 1) with row stride % 4 == 0. One entry per refusal (gen-*), each on
                                k_vm_eval_generic with 0 generated launches; three axes below 2^16 elements (the axes forms
                                refuse) and eight uncollapsible axes as well. One grid trip of the generic kernel is 2048 * 256 =
                                524288 elements: gen-second-trip (gpu only).
  spec_modes                    LM_VEC unit stride | LM_ROWB inner stride 0, row stride != 0: the (R, 1) leaf | LM_CONST both 0:
                                one device element | LM_ROWINV (SWEEP only) unit stride, row stride 0: the (C,) leaf, which is
                                LM_VEC everywhere else. Program `d4` takes one leaf of each in one entry per form.
  full reduction                gridDim.x < 64: md_ticket_last; >= 64: md_ticket_last2, arrival i on shard i % 32 — 64 blocks: two
                                per shard; 65: shard 0 has three; 97: shard 0 has four, the others three. max_blocks 1 / 3 / 63 /
                                64 / 65 / 97 at 4 * (256 * cap + 5) + 3 elements fill the cap in both legs (lanes 0 .. 4 a second
                                trip). md_fold_partials: thread t folds partials t, t + 256, ..: one each up to 256 blocks; at the
                                default caps 2^21 + 7 elements give the interpreter 2048 blocks (eight partials per lane), RED_ALL
                                1024 (four): redall-default-caps (gpu only).
  reduce_cols_2d, tiled         bx = ceil(n_out / 256); splits = clamp(min(1024 / bx, n_red / 32), 1, 65535); chunk = ceil(ceil(
                                n_red / splits) / 16) * 16; splits = ceil(n_red / chunk). n_out 260: n_red 1 .. 63 -> 1 split (`out`
                                written directly), 64 -> 2 x 32, 65 -> 2 chunks of 48 (the last holds 17 rows), 100 -> 3 (last 4),
                                511 -> 11 (last 31), 512 -> 16 x 32, 513 -> 11 x 48, 2000 -> 42 x 48; the second pass runs
                                k_vm_reduce_cols over the `splits` partial rows with chunk2 = ceil(splits / 16) * 16 > splits except
                                at 512. The generated leg takes RED_COLS below n_red 512 and the strips kernel from there on (one
                                launch either way; the second pass is always the interpreter kernel). Dense leaves collapse to one
                                axis and go through uncollapse_2d; a padded pitch (% 4 == 0), a (C,) or a (R, 1) leaf keep two.
                                The interpreter's lane row takes rows r0 + ry, + 4, ..; RED_COLS two of them per trip while
                                row + 4 < r1, then one: chunks of 1 .. 17 rows cover both loops with 0, 1 and 2 trips.
  sweep_cols / sweep_geometry   n_red >= 512, n_out % 4 == 0; NS = ceil(n_out / 256) strips; NB = sweep_nb or 256 / NS, clamped to
                                [1, min(64, n_red / (4 RU))]; RU = sweep_ru or ceil(128 / row bytes) <= 8. Wave w of band b takes
                                rows b + NB w + 4 NB i: nrw = ceil((n_red - first) / (4 NB)) rows in nbt = nrw / RU pipelined batches
                                + nrw % RU single rows. NB 64, RU 2: n_red 512 -> nbt 1; 513 -> 1 (+ 1 row in one wave); 1025 -> 2
                                (+ 1); 1537 -> 3 (+ 1); 2048 -> 4; 2049 -> 4 (+ 1); 700 -> waves of 3 and of 2 rows. The pipeline's
                                loop runs floor(nbt / 2) times and one more batch when nbt is odd: nbt 1, 2, 3, 4 are its four
                                shapes. NB 1 / RU 1 (512: 128 batches), NB 2 / RU 1, NB 3 / RU 8 (512: nrw 42 / 43 -> 5 batches + 2 / 3
                                rows; 777: 64 / 65 -> 8 + 0 / 1), NB 1 / RU 8 (515), and the default band count (640 x 64: NB = min(64,
                                640 / (4 RU))). n_out 4 (one lane stores), 252 (ragged: lane 63 computes c = n_out - 4, stores
                                nothing), 256, 260 (second strip: one lane), 516 (three strips). NB > 1: partial rows + one ticket per
                                strip; NB = 1: direct store. The `store` form (mdhip_vm_eval_reduce_cols) is the same kernel; it has
                                no interpreter form: with jit = 0 the call returns an error and _materialize evaluates and reduces
                                in two passes, which is what the interpreter leg of the evalcols-* entries asserts.
  vm_eval_multi                 merge_programs gives identical leaf descriptors ONE slot and every immediate a slot of its own;
                                declined (then one mdhip_vm_eval per program, counted): jit = 0, an output that is not of the
                                compute dtype, outputs of different strides, an output off 16 bytes.

Not reachable at test size (no entry pretends otherwise): the 64-bit division of vm_row_col / JPos::init (2^32 groups); a row count
that overflows the strips kernel's 32-bit buffer offsets (NB * n_out * 8 bytes >= 2^32); gridDim.y > 65535 in the tiled kernel
(n_red >= 2^21 rows); nbt = 0 in the strips kernel (NB <= n_red / (4 RU) gives every wave at least RU rows); the non-temporal variants
(more than 320 MiB streamed; no option forces them); a leaf table that overflows in merge_programs (lazy.py batches at most eight
distinct leaves).

Programs (a generated kernel is keyed by program, leaf modes and shape parameters — not by sizes or constants: the geometry sweeps
reuse compilations): `two` c0 * x - y / c1 (a constant on each side); `where` where(m, x, y) with a bool leaf; `sincos` sin(x) *
cos(x) + y (the hoisted sincos); `d4` (x + z) * (y * z + (x - w) * (y + w)) at stack depth 4; `eight` (a + b) * (c - d) + (e * f -
g * h), 8 leaves; `long44` ((x * y + c0 - c1 ...) * z), 44 instructions — the most lazy.py builds, the interpreter's LDS staging
full; `m2` (x + c0) * (y - c1), `m3` where(m, x * c0, y), `m4` y * c0 / (x * x + c1) next to `two` in the multi-output entries.

Data and references — every comparison is on raw bits (a NaN matches any NaN) or on exactly representable results; no tolerance:
  evaluations   normals * 10^uniform(-3, 3) with NaN, +-inf, +-0.0 and a subnormal planted (in the leaves of the program's own
                shape, one leaf per position) at element 0, both sides of the last whole vector, every tail element and both
                sides of every grid-trip boundary. Reference: the SAME chain evaluated eagerly on the same build, and NumPy's bits
                where NumPy is correctly rounded (+ - * /, where: every program but sincos). bool outputs: value != 0 (half the
                operands' elements are zeros there); float16 outputs: NumPy's astype(float16) of the eager chain (gpu only: the
                double refuses float16 outputs, tests/test_fused_narrow.py).
  sums          integers hashed from the element index, the widest of 20 .. 1 bits at which the sum of magnitudes of every reduced
                slice stays below 2^53 (float64) / 2^24 (float32): exact in any order; a dropped element and a duplicated one
                cannot cancel. Programs in which a roll of one leaf changes the sum: where, d4, eight, long44.
  products      where(m, x, y) over +-1 with a handful of 2s and halves per reduced slice.
  max / min     a permutation per leaf; then one run per structural position (first, last, a tail element or the first row of the last chunk /
                band, the last column group of a ragged strip) with the extreme +-1e30 planted there, and one with a NaN.
  reductions    reference: NumPy on the eagerly evaluated chain; every call is made twice and must give the same bits; the store
                form's evaluated chain is compared with the eager bits as well.
Position sensitivity (CPU twin): rolling any array leaf by one along any of its axes longer than 1 changes the reference of every
entry (max / min: of the run without a planted extreme).

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound; it proves data and references and runs the
sensitivity check) and gpu-marked on the product library, both legs. test_public runs a subset through nd.* with lazy mode on.
Not run on both twins: the float16 outputs and the three entries at the default grids (2^21 + 7 and 2^19 + 300 elements say nothing
on the double, which has one loop); the refusals at the C-ABI are the product launchers' own (the double runs two plain loops
where they refuse) — the same shapes through nd.* run on both.

Found with it: nothing in the kernels — every entry passes on the library as it was."""
import ctypes as C
import zlib

import numpy as np
import pytest

from minidiff_amd import _capi

from test_fused_axis import _nb, _ru      # the strips kernel's geometry, as derived there
from test_fused_narrow import _eager, _same

gpu = pytest.mark.gpu
f16, f32, f64, b8 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.bool_)
PAD = 16            # sentinel elements in front of and behind every view: a multiple of 16 B for every element size
SENT = -777.0       # output sentinel (exact in float16); bool outputs: the byte 0x5A
T = 768             # grid stride in vector groups under max_blocks = 3
MB3 = {"max_blocks": 3}
CODES = {"sum": _capi.R_SUM, "prod": _capi.R_PROD, "max": _capi.R_MAX, "min": _capi.R_MIN}
BIG = 1e30


# ------------------------------------------------------------------------------------------------------------------------- programs
class _NP:
    """NumPy under the names the programs use"""
    add, subtract, multiply, true_divide, where, sin, cos = np.add, np.subtract, np.multiply, np.true_divide, np.where, np.sin, np.cos


def _p_two(o, c, x, y):
    return o.subtract(o.multiply(c[0], x), o.true_divide(y, c[1]))


def _p_where(o, c, m, x, y):
    return o.where(m, x, y)


def _p_sincos(o, c, x, y):
    return o.add(o.multiply(o.sin(x), o.cos(x)), y)


def _p_d4(o, c, x, y, z, w):
    return o.multiply(o.add(x, z), o.add(o.multiply(y, z), o.multiply(o.subtract(x, w), o.add(y, w))))


def _p_eight(o, c, a, b, cc, d, e, f, g, h):
    return o.add(o.multiply(o.add(a, b), o.subtract(cc, d)), o.subtract(o.multiply(e, f), o.multiply(g, h)))


def _p_long44(o, c, x, y, z):
    t = o.multiply(x, y)
    for _ in range(21):
        t = o.subtract(o.add(t, c[0]), c[1])
    return o.multiply(t, z)


def _p_m2(o, c, x, y):
    return o.multiply(o.add(x, c[0]), o.subtract(y, c[1]))


def _p_m3(o, c, m, x, y):
    return o.where(m, o.multiply(x, c[0]), y)


def _p_m4(o, c, x, y):
    return o.true_divide(o.multiply(y, c[0]), o.add(o.multiply(x, x), c[1]))


# name -> (function, parameter names, NumPy is correctly rounded, (instructions, stack depth), the leaves that carry a planted extreme)
PROGS = {
    "two": (_p_two, ("x", "y"), True, (3, 2), ("x",)),
    "where": (_p_where, ("m", "x", "y"), True, (4, 3), ("x", "y")),
    "sincos": (_p_sincos, ("x", "y"), False, (6, 2), ("y",)),
    "d4": (_p_d4, ("x", "y", "z", "w"), True, (7, 4), ()),
    "eight": (_p_eight, ("a", "b", "c", "d", "e", "f", "g", "h"), True, (7, 3), ()),
    "long44": (_p_long44, ("x", "y", "z"), True, (44, 1), ()),
    "m2": (_p_m2, ("x", "y"), True, (3, 2), ()),
    "m3": (_p_m3, ("m", "x", "y"), True, (4, 3), ()),
    "m4": (_p_m4, ("x", "y"), True, (4, 2), ()),
}
C_EVAL, C_RED = (0.75, 3.0), (2.0, 0.5)      # constants of the evaluations / of the reductions (integers stay integers)
C_LONG_RED = (3.0, 2.0)


# --------------------------------------------------------------------------------------------------------------------------- layout
class V:
    """A view cut from a 1-D base: `keep` None — the program's shape; a tuple of flags — extent 1 where False ((False, True): the (C,)
    leaf as (1, C); (True, False): (R, 1); all False: one device element behind a stride-0 view). From element `off`, inner stride
    `step`, row pitch `pitch` (2-D), `perm`: the axes' order in memory. `share`: views with one key are cut from ONE base at one
    offset (the leaf that appears with two strides). dt: bool for the mask."""

    def __init__(self, keep=None, off=PAD, pitch=None, step=1, perm=None, share=None, dt=None):
        self.keep, self.off, self.pitch, self.step, self.perm, self.share, self.dt = keep, off, pitch, step, perm, share, dt

    def lshape(self, shape):
        return tuple(shape) if self.keep is None else tuple(s if k else 1 for s, k in zip(shape, self.keep))

    def strides(self, shape):
        ls = self.lshape(shape)
        order = list(self.perm) if self.perm else list(range(len(ls)))      # order[-1] is the fastest axis
        st, run = [0] * len(ls), self.step
        for k, ax in enumerate(reversed(order)):
            st[ax] = run
            run = self.pitch * self.step if (k == 0 and self.pitch) else run * ls[ax]
        return tuple(st)

    def span(self, shape):
        return 1 + sum((e - 1) * s for e, s in zip(self.lshape(shape), self.strides(shape)))

    def cut(self, base, shape):
        """the NumPy view"""
        ls, st = self.lshape(shape), self.strides(shape)
        return np.lib.stride_tricks.as_strided(base[self.off:], ls, tuple(s * base.itemsize for s in st))

    def dcut(self, dbase, shape):
        """the device view"""
        return dbase._view(self.off, self.lshape(shape), self.strides(shape))


ROW, COL, ONE = (False, True), (True, False), (False, False)
FULL = lambda: V()      # noqa: E731


class Entry:
    """form: eval | reduce (full) | cols (vm_reduce over axis 0) | evalcols (vm_eval_reduce_cols) | multi. progs: [(program, [leaf
    names])]. outs: one V per program (evaluations; cols / evalcols: [evaluated, reduced]). launches: generated launches of ONE call
    in the generated leg (the interpreter leg makes none). odt: None — the compute dtype. trips: grid strides in vector groups."""

    def __init__(self, id, reaches, form, shape, progs, leaves, outs, cdt=f32, odt=None, op=None, opts=None, launches=1, gpu_only=False,
                 no_double=False, trips=(), positions=(), public=False, consts=None):
        self.id, self.reaches, self.form, self.shape, self.progs, self.leaves, self.outs = id, reaches, form, tuple(shape), progs, leaves, outs
        self.cdt, self.odt, self.op, self.opts, self.launches = cdt, np.dtype(odt) if odt is not None else cdt, op, dict(opts or {}), launches
        self.gpu_only, self.no_double, self.trips, self.positions, self.public = gpu_only, no_double or gpu_only, tuple(trips), tuple(positions), public
        self.consts = consts or (C_EVAL if form in ("eval", "multi") else C_RED)
        self.n = int(np.prod(self.shape, dtype=np.int64))

    @property
    def red_shape(self):
        return (1,) if self.form == "reduce" else (1, self.shape[1])


TABLE = []


def _e(id, reaches, form, shape, prog, leaves, out=None, **k):
    names = PROGS[prog][1]
    assert len(names) == len(leaves), id
    lv = {n: s for n, s in zip(names, leaves)}
    if "m" in lv:
        lv["m"].dt = b8
    if prog == "long44" and form not in ("eval", "multi"):
        k.setdefault("consts", C_LONG_RED)
    outs = [out or V()] if form in ("eval", "reduce") else [out or V(), V()]
    TABLE.append(Entry(id, reaches, form, shape, [(prog, list(names))], lv, outs, **k))


def _leaves(prog, mode="full", pitch=None):
    """full: every leaf of the program's shape; row: the last array leaf a (C,) one; pitch: the last one with a padded row pitch;
    modes: x full, y (C,), z (R, 1), w one element"""
    names = PROGS[prog][1]
    if mode == "modes":
        assert prog == "d4"
        return [V(), V(ROW), V(COL), V(ONE)]
    lv = [V() for _ in names]
    if mode == "row":
        lv[-1] = V(ROW)
    if mode == "pitch":
        lv[-1] = V(pitch=pitch)
    return lv


# ---- evaluations, (rows, inner): k_vm_eval_fast / EVAL --------------------------------------------------------------------------
FAST = "k_vm_eval_fast | EVAL (k_fused_eval*)"
_TAILS = {0: (1, 2, 3), 1: (0, 1, 2, 3), 767: (3,), 768: (0,), 769: (0, 1, 2, 3), 1535: (1,), 1536: (2,), 1537: (0, 1, 2, 3), 2305: (3,), 3073: (1,)}
for _nv, _ts in _TAILS.items():
    for _t in _ts:
        _n = 4 * _nv + _t
        if _n == 1:
            _e("eval-1d-nv0+1", "k_vm_eval_generic: one element collapses to zero axes (both legs)", "eval", (1,), "two", _leaves("two"), opts=MB3, launches=0)
            continue
        _e(f"eval-1d-nv{_nv}+{_t}", f"{FAST}, 1-D: {_nv} groups, tail {_t}", "eval", (_n,), "two", _leaves("two"), opts=MB3, trips=(T,),
           cdt=f64 if _nv in (1, 1537) else f32, public=(_nv, _t) in ((769, 3), (1537, 1)))
for _u in (1, 3, 4):
    for _k in (3, 4):
        _e(f"eval-1d-u{_u}-{_k}T+1", f"EVAL with U = {_u} at {_k} * 768 + 1 groups | k_vm_eval_fast", "eval", (4 * (_k * T + 1) + 1,), "two", _leaves("two"),
           opts=dict(MB3, jit_u=_u), trips=(T,))
_e("eval-1d-default-grid", f"{FAST}: the default grids, a second trip (1024 blocks generated, 2048 interpreter)", "eval", ((1 << 21) + 7,), "two", _leaves("two"),
   trips=(1024 * 256, 2048 * 256), gpu_only=True)
_e("eval-1d-bool-out", f"{FAST}: bool output (k_fused_evalb)", "eval", (4 * 769 + 3,), "two", _leaves("two"), opts=MB3, trips=(T,), odt=b8)
_e("eval-1d-f16-out", f"{FAST}: float16 output (k_fused_evalh)", "eval", (4 * 769 + 3,), "two", _leaves("two"), opts=MB3, trips=(T,), odt=f16, no_double=True)
for _p, _dt in (("where", f32), ("sincos", f32), ("eight", f64), ("long44", f32)):
    _e(f"eval-1d-{_p}", f"{FAST}, 1-D, program {_p}", "eval", (4 * 1537 + 3,), _p, _leaves(_p), opts=MB3, trips=(T,), cdt=_dt, public=_p in ("where", "long44"))
_e("eval-1d-d4-const", f"{FAST}, 1-D, stack depth 4, w one device element (LM_CONST)", "eval", (4 * 1537 + 3,), "d4", [V(), V(), V(), V((False,))],
   opts=MB3, trips=(T,), cdt=f64)
_e("eval-1d-sincos-const", f"{FAST}, 1-D, sin / cos of one device element (hoisted in the prologue)", "eval", (4 * 769 + 2,), "sincos", [V((False,)), V()],
   opts=MB3, trips=(T,))
_2D = ((400, 20), (331, 28), (3, 3072), (3, 4000))
for _s in _2D:
    _e(f"eval-2d-{_s[0]}x{_s[1]}", f"{FAST}, 2-D: nv {_s[1] // 4}, (dq, dr) = {divmod(T, _s[1] // 4)}", "eval", _s, "two", _leaves("two", "row"), opts=MB3,
       trips=(T,), cdt=f64 if _s[1] == 28 else f32, public=_s[1] == 20)
_e("eval-2d-modes", f"{FAST}, 2-D: LM_VEC, (C,), LM_ROWB, LM_CONST in one program of depth 4", "eval", (331, 28), "d4", _leaves("d4", "modes"), opts=MB3, trips=(T,), public=True)
_e("eval-2d-pitch", f"{FAST}, 2-D: a leaf with a padded row pitch", "eval", (400, 20), "two", [V(pitch=24), V()], opts=MB3, trips=(T,))
_e("eval-2d-bool-out", f"{FAST}, 2-D: bool output, bool leaf", "eval", (400, 20), "where", _leaves("where", "row"), opts=MB3, trips=(T,), odt=b8)
_e("eval-2d-f16-out", f"{FAST}, 2-D: float16 output", "eval", (400, 20), "two", _leaves("two", "row"), opts=MB3, trips=(T,), odt=f16, no_double=True)
_e("eval-2d-sincos-row", f"{FAST}, 2-D: sin / cos of a (C,) leaf", "eval", (400, 20), "sincos", [V(ROW), V()], opts=MB3, trips=(T,))
_e("eval-2d-sincos-col", f"{FAST}, 2-D: sin / cos of a (R, 1) leaf (LM_ROWB: once per group)", "eval", (400, 20), "sincos", [V(COL), V()], opts=MB3, trips=(T,))

# ---- evaluations, any strides: k_vm_eval_generic (no generated form) -----------------------------------------------------------
GEN = "k_vm_eval_generic"
_e("gen-inner-odd", f"{GEN}: rows > 1, inner % 4 != 0", "eval", (7, 10), "two", _leaves("two", "row"), launches=0)
_e("gen-leaf-misaligned", f"{GEN}: a leaf one element off its alignment", "eval", (1024,), "two", [V(off=PAD + 1), V()], launches=0)
_e("gen-row-stride-odd", f"{GEN}: row stride % 4 != 0", "eval", (8, 16), "two", [V(pitch=18), V()], launches=0)
_e("gen-inner-stride-2", f"{GEN}: inner stride 2", "eval", (1024,), "two", [V(step=2), V()], launches=0, public=True)
_e("gen-out-pitch", f"{GEN}: output rows not dense", "eval", (8, 16), "two", _leaves("two"), out=V(pitch=20), launches=0)
_e("gen-out-step-2", f"{GEN}: output stride 2", "eval", (1024,), "two", _leaves("two"), out=V(step=2), launches=0)
_e("gen-out-misaligned", f"{GEN}: output one element off its alignment", "eval", (1024,), "two", _leaves("two"), out=V(off=PAD + 1), launches=0)
_e("gen-3-axes-small", f"{GEN}: three axes below 65536 elements (the axes forms refuse)", "eval", (5, 6, 8), "two", [V(), V((True, False, True))], launches=0)
_e("gen-8d", f"{GEN}: eight axes, a leaf with its axes reversed in memory", "eval", (2,) * 8, "two", [V(perm=tuple(range(7, -1, -1))), V()], launches=0)
_e("gen-second-trip", f"{GEN}: above 2048 * 256 elements, a second grid trip", "eval", (2048 * 256 + 300,), "two", [V(step=2), V()], launches=0, gpu_only=True)
_e("gen-bool-out", f"{GEN}: bool output", "eval", (1027,), "where", [V(), V(step=2), V()], launches=0, odt=b8)
_e("gen-f16-out", f"{GEN}: float16 output", "eval", (1027,), "two", [V(step=2), V()], launches=0, odt=f16, no_double=True)
_e("gen-d4-modes", f"{GEN}: depth 4, the four leaf geometries", "eval", (7, 10), "d4", _leaves("d4", "modes"), launches=0, cdt=f64)
_e("gen-long44", f"{GEN}: 44 instructions", "eval", (7, 10), "long44", _leaves("long44", "row"), launches=0)
_e("gen-sincos", f"{GEN}: sin and cos", "eval", (7, 10), "sincos", _leaves("sincos", "row"), launches=0)
_e("gen-eight", f"{GEN}: 8 leaves", "eval", (1027,), "eight", [V(step=2)] + [V() for _ in range(7)], launches=0)

# ---- full reductions: k_vm_reduce_all / RED_ALL -----------------------------------------------------------------------------------
ALL = "k_vm_reduce_all | RED_ALL (k_fused_redall)"
for _cap in (1, 3, 63, 64, 65, 97):
    _e(f"redall-cap{_cap}", f"{ALL}: {_cap} blocks, {'md_ticket_last' if _cap < 64 else 'md_ticket_last2'}", "reduce", (4 * (256 * _cap + 5) + 3,), "where",
       _leaves("where"), op="sum", opts={"max_blocks": _cap}, public=_cap == 65)
for _nv, _ts in _TAILS.items():
    for _t in _ts:
        if 4 * _nv + _t > 1:
            _e(f"redall-1d-nv{_nv}+{_t}", f"{ALL}, 1-D: {_nv} groups, tail {_t}", "reduce", (4 * _nv + _t,), "where", _leaves("where"), op="sum", opts=MB3,
               cdt=f64 if _nv in (1, 1537) else f32)
for _s in _2D:
    _e(f"redall-2d-{_s[0]}x{_s[1]}", f"{ALL}, 2-D: nv {_s[1] // 4}", "reduce", _s, "where", _leaves("where", "row"), op="sum", opts=MB3, cdt=f64 if _s[1] == 28 else f32)
_e("redall-2d-modes", f"{ALL}, 2-D: the four leaf modes, depth 4", "reduce", (331, 28), "d4", _leaves("d4", "modes"), op="sum", opts=MB3)
_e("redall-1d-eight", f"{ALL}: 8 leaves", "reduce", (4 * 1537 + 3,), "eight", _leaves("eight"), op="sum", opts=MB3, cdt=f64)
_e("redall-1d-long44", f"{ALL}: 44 instructions", "reduce", (4 * 1537 + 3,), "long44", _leaves("long44"), op="sum", opts=MB3, public=True)
_e("redall-1d-prod", f"{ALL}: prod", "reduce", (4 * 1537 + 3,), "where", _leaves("where"), op="prod", opts=MB3)
_e("redall-2d-prod", f"{ALL}, 2-D: prod", "reduce", (400, 20), "where", _leaves("where", "pitch", 24), op="prod", opts=MB3, cdt=f64)
for _op in ("max", "min"):
    _n = 4 * 3073 + 3
    _e(f"redall-1d-{_op}", f"{ALL}: {_op}, the extreme / a NaN at the first, the last (a tail) element, both sides of a trip boundary", "reduce", (_n,), "two",
       _leaves("two"), op=_op, opts=MB3, positions=(0, _n - 1, 4 * 3072, 4 * T - 1, 4 * T), public=_op == "max")
_e("redall-2d-max-sincos", f"{ALL}, 2-D: max of the sincos program (hoisted sin / cos in a reduction)", "reduce", (331, 28), "sincos", _leaves("sincos", "pitch", 32),
   op="max", opts=MB3, positions=(0, 331 * 28 - 1))
_e("redall-default-caps", f"{ALL}: the default caps (2048 / 1024 blocks), md_fold_partials with eight / four partials per lane", "reduce", ((1 << 21) + 7,), "where",
   _leaves("where"), op="sum", gpu_only=True)

# ---- axis 0 of a 2-D program, tiled: k_vm_reduce_cols (+ second pass) / RED_COLS -----------------------------------------------
COLS = "k_vm_reduce_cols | RED_COLS (k_fused_redcols)"


def _splits(n_red, n_out):
    """reduce_cols_2d: -> (splits, chunk)"""
    bx = -(-n_out // 256)
    splits = max(1, min(1024 // bx, n_red // 32, 65535))
    chunk = -(-(-(-n_red // splits)) // 16) * 16
    return -(-n_red // chunk), chunk


def _cols_reach(n_red, n_out):
    s, c = _splits(n_red, n_out)
    second = f", second pass over {s} partial rows (chunk2 {-(-s // 16) * 16})" if s > 1 else ", `out` written directly"
    strips = "; generated leg: SWEEP (k_fused_sweepcols)" if n_red >= 512 else ""
    return f"{COLS if n_red < 512 else 'k_vm_reduce_cols'}: {s} x {c} rows (last {n_red - (s - 1) * c}){second}{strips}"


for _r in (1, 4, 31, 32, 33, 63, 64, 65, 100, 511, 512, 513, 2000):
    _e(f"cols-{_r}x260", _cols_reach(_r, 260) + "; dense leaves: uncollapse_2d", "cols", (_r, 260), "where", _leaves("where"), op="sum", public=_r in (65, 2000))
for _c in (4, 252, 256, 516, 1028):
    for _r in (33, 100):
        _e(f"cols-{_r}x{_c}", _cols_reach(_r, _c) + "; dense leaves", "cols", (_r, _c), "where", _leaves("where"), op="sum")
_e("cols-100x260-pitch", _cols_reach(100, 260) + "; a padded row pitch keeps two axes", "cols", (100, 260), "where", [V(), V(pitch=264), V()], op="sum")
_e("cols-65x516-pitch", _cols_reach(65, 516) + "; a padded row pitch", "cols", (65, 516), "where", [V(pitch=520), V(), V()], op="sum")
_e("cols-100x260-row", _cols_reach(100, 260) + "; a (C,) leaf", "cols", (100, 260), "where", _leaves("where", "row"), op="sum", public=True)
_e("cols-100x260-modes", _cols_reach(100, 260) + "; the four leaf modes, depth 4", "cols", (100, 260), "d4", _leaves("d4", "modes"), op="sum")
_e("cols-511x260-f64", _cols_reach(511, 260) + "; float64", "cols", (511, 260), "where", _leaves("where"), op="sum", cdt=f64)
_e("cols-100x260-eight", _cols_reach(100, 260) + "; 8 leaves", "cols", (100, 260), "eight", _leaves("eight"), op="sum", cdt=f64)
_e("cols-100x260-long44", _cols_reach(100, 260) + "; 44 instructions", "cols", (100, 260), "long44", _leaves("long44", "row"), op="sum")
_e("cols-100x260-prod", _cols_reach(100, 260) + "; prod", "cols", (100, 260), "where", _leaves("where"), op="prod")
for _op in ("max", "min"):
    # 100 rows: chunks of 48, the last one starts at row 96; n_out 260: the second block's only column group is columns 256 .. 259
    _e(f"cols-100x260-{_op}", _cols_reach(100, 260) + f"; {_op}: the extreme / a NaN at the first and the last element, the first row of the last chunk, the ragged block",
       "cols", (100, 260), "two", _leaves("two", "pitch", 264), op=_op, positions=(0, 100 * 260 - 1, 96 * 260 + 5, 50 * 260 + 256))

# ---- axis 0 of a 2-D program, strips: SWEEP, and SWEEP with store ---------------------------------------------------------------


def _sweep_reach(n_red, n_out, nb, ru, vec_sizes):
    RU = ru or _ru(vec_sizes)
    NB = _nb(1, n_red, n_out, RU, nb)
    nrw = sorted({-(-(n_red - f) // (4 * NB)) for f in range(4 * NB)})
    return (f"NS {-(-n_out // 256)}, NB {NB}, RU {RU}: waves of {' / '.join(map(str, nrw))} rows, nbt {' / '.join(str(r // RU) for r in nrw)}"
            f" + {' / '.join(str(r % RU) for r in nrw)} single rows"), NB, RU, nrw


def _sweep(tag, n_red, n_out, nb, ru, prog="where", mode="full", op="sum", cdt=f32, store=True, **k):
    sizes = [1 if n == "m" else cdt.itemsize for n, s in zip(PROGS[prog][1], _leaves(prog, mode, n_out + 4)) if s.keep is None]
    what, NB, RU, nrw = _sweep_reach(n_red, n_out, nb, ru, sizes)
    opts = {}
    if nb:
        opts["sweep_nb"] = nb
    if ru:
        opts["sweep_ru"] = ru
    _e(f"sweep-{tag}", f"SWEEP (k_fused_sweepcols): {what} | interpreter leg: k_vm_reduce_cols", "cols", (n_red, n_out), prog, _leaves(prog, mode, n_out + 4), op=op, cdt=cdt, opts=opts, **k)
    if store:
        k.pop("public", None)
        _e(f"evalcols-{tag}", f"SWEEP with store (k_fused_evalcols): {what} | interpreter leg: the C-ABI refuses", "evalcols", (n_red, n_out), prog, _leaves(prog, mode, n_out + 4), op=op,
           cdt=cdt, opts=opts, **k)


for _r in (512, 513, 1025, 1537, 2048, 2049, 700):
    _sweep(f"nb64-ru2-{_r}x260", _r, 260, 64, 2, public=_r == 700)
for _c in (4, 252, 256, 516):
    _sweep(f"nb64-ru2-700x{_c}", 700, _c, 64, 2)
_sweep("nb1-ru1-512x260", 512, 260, 1, 1)
_sweep("nb2-ru1-513x260", 513, 260, 2, 1)
_sweep("nb3-ru8-512x260", 512, 260, 3, 8)
_sweep("nb3-ru8-777x252", 777, 252, 3, 8)
_sweep("nb1-ru8-515x260", 515, 260, 1, 8)
_sweep("nb2-ru2-640x516", 640, 516, 2, 2)
_sweep("default-640x64", 640, 64, 0, 0, public=True)
_sweep("nb64-ru2-700x260-rowinv", 700, 260, 64, 2, mode="row")
_sweep("nb3-ru8-777x260-modes", 777, 260, 3, 8, prog="d4", mode="modes")
_sweep("nb64-ru2-1025x260-f64", 1025, 260, 64, 2, cdt=f64)
_sweep("nb64-ru2-700x260-eight", 700, 260, 64, 2, prog="eight", cdt=f64, store=False)
_sweep("nb64-ru2-700x260-long44", 700, 260, 64, 2, prog="long44", mode="row", store=False)
_sweep("nb64-ru2-700x260-prod", 700, 260, 64, 2, op="prod")
for _op in ("max", "min"):
    # NB 64 <= 700 / 8: the last band is band 63, its first row is row 63; n_out 252: lane 63 of the strip is past the edge, the last
    # column group is columns 248 .. 251
    _sweep(f"nb64-ru2-700x252-{_op}", 700, 252, 64, 2, prog="two", mode="pitch", op=_op, positions=(0, 700 * 252 - 1, 63 * 252 + 9, 699 * 252 + 248))
_sweep("nb64-ru2-700x252-max-sincos", 700, 252, 64, 2, prog="sincos", mode="full", op="max", positions=(0, 350 * 252 + 251), store=False)

# ---- several outputs, one launch: merged EVAL ------------------------------------------------------------------------------------
MULTI = "merged EVAL (k_fused_eval{n})"


def _m(id, reaches, shape, progs, leaves, outs=None, **k):
    for n, s in leaves.items():
        if n == "m":
            s.dt = b8
    TABLE.append(Entry(id, reaches, "multi", shape, progs, leaves, outs or [V() for _ in progs], **k))


_XY, _MXY = ["x", "y"], ["m", "x", "y"]
_M2, _M3, _M4 = [("two", _XY), ("m2", _XY)], [("two", _XY), ("m2", _XY), ("m3", _MXY)], [("two", _XY), ("m2", _XY), ("m3", _MXY), ("m4", _XY)]
for _t in range(4):
    _m(f"multi-2-1d-tail{_t}", MULTI.format(n=2) + f": shared leaves x, y; 1-D, tail {_t} | interpreter leg: k_vm_eval_fast per program", (4 * 769 + _t,), _M2,
       {"x": V(), "y": V()}, opts=MB3, trips=(T,), public=_t == 3)
_m("multi-3-1d", MULTI.format(n=3) + ": x, y shared by three programs, m by one", (4 * 1537 + 1,), _M3, {"m": V(), "x": V(), "y": V()}, opts=MB3, trips=(T,))
_m("multi-4-1d-f64", MULTI.format(n=4) + ": float64", (4 * 1537 + 2,), _M4, {"m": V(), "x": V(), "y": V()}, opts=MB3, trips=(T,), cdt=f64)
_m("multi-3-2d", MULTI.format(n=3) + ": 2-D, nv 5, y a (C,) leaf", (400, 20), _M3, {"m": V(), "x": V(), "y": V(ROW)}, opts=MB3, trips=(T,), public=True)
_m("multi-2-2d", MULTI.format(n=2) + ": 2-D, nv 7, float64", (331, 28), _M2, {"x": V(), "y": V(ROW)}, opts=MB3, trips=(T,), cdt=f64)
_m("multi-2-2d-modes", MULTI.format(n=2) + ": the four leaf modes (LM_VEC, (C,), LM_ROWB, LM_CONST), depth 4 next to a program that shares x and y", (331, 28),
   [("d4", ["x", "y", "z", "w"]), ("m2", _XY)], {"x": V(), "y": V(ROW), "z": V(COL), "w": V(ONE)}, opts=MB3, trips=(T,))
_m("multi-2-two-strides", MULTI.format(n=2) + ": ONE buffer as a (C,) leaf of one program and as a (R, 1) leaf of the other: two slots", (20, 20),
   [("two", ["x", "vr"]), ("m2", ["x", "vc"])], {"x": V(), "vr": V(ROW, share="v"), "vc": V(COL, share="v")}, opts=MB3)
_m("multi-declined-bool", "declined (a bool output): one EVAL (k_fused_evalb) per program", (4 * 769 + 3,),
   [("two", _XY), ("m3", _MXY)], {"m": V(), "x": V(), "y": V()}, opts=MB3, trips=(T,), odt=b8, launches=2)
_m("multi-declined-strides", "declined (outputs of different strides): EVAL for the dense one, k_vm_eval_generic for the other", (8, 16), _M2, {"x": V(), "y": V()},
   outs=[V(), V(pitch=20)], launches=1)
_m("multi-declined-misaligned", "declined (an output off 16 bytes): EVAL for the aligned one, k_vm_eval_generic for the other", (1024,), _M2, {"x": V(), "y": V()},
   outs=[V(), V(off=PAD + 1)], launches=1)

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)


# ----------------------------------------------------------------------------------------------------------------------------- data
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def _marks(e):
    """flat positions of the specials: element 0, both sides of the last whole vector, every tail element, both sides of every
    grid-trip boundary"""
    n, n4 = e.n, e.n // 4 * 4
    P = [0, 3, 4, n4 - 5, n4 - 4, n4 - 1, n - 1] + list(range(n4, n))
    for t in e.trips:
        for b in range(4 * t, n, 4 * t):
            P += [b - 1, b]
    return sorted({p for p in P if 0 <= p < n})


def _hash_ints(size, bits, salt):
    h = (np.arange(size, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x9E3779B9 * (salt + 1))) & np.uint64(0xFFFFFFFF)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(32 - bits)).astype(np.int64) - (1 << (bits - 1))


_DRAWS = {}


def _draw_of(e):
    """A handful of elements can be their own rolled copy by chance: the data of a small entry is the first draw, in a fixed order of
    seeds, that is position sensitive (the CPU twin asserts the condition for every size)."""
    if e.id not in _DRAWS:
        _DRAWS[e.id] = 0
        # (.. and a product of a few non-units, which a roll changes with a probability well below one)
        if sum(int(np.prod(s.lshape(e.shape), dtype=np.int64)) for s in e.leaves.values()) <= 4096 or (e.op == "prod" and e.n < (1 << 18)):
            for draw in range(64):
                if not Data(e, None, draw).insensitive():
                    _DRAWS[e.id] = draw
                    break
    return _DRAWS[e.id]


class Data:
    """The leaves of one entry as NumPy views inside their bases, the references, the expected output bases. `plant`: None, or (flat
    position, "ext" | "nan") for max / min."""

    def __init__(self, e, plant=None, draw=None):
        self.e = e
        self.draw = draw = _draw_of(e) if draw is None else draw
        rng = np.random.default_rng([zlib.crc32(e.id.encode()), 7, draw])
        shape, cdt = e.shape, e.cdt
        full_float = [n for n, s in e.leaves.items() if s.dt is None and s.lshape(shape) == shape]
        vals, shared = {}, {}
        red = e.form != "eval" and e.form != "multi"
        bits = None
        if red and e.op == "sum":
            for bits in (20, 16, 12, 10, 8, 6, 5, 4, 3, 2, 1):
                vals = self._sum_values(bits)
                if self._sum_fits(vals):
                    break
            else:
                raise AssertionError((e.id, "no exact sum data"))
        for k, (name, s) in enumerate(e.leaves.items()):
            ls = s.lshape(shape)
            size = int(np.prod(ls, dtype=np.int64))
            if name in vals:
                continue
            if s.share and s.share in shared:
                vals[name] = shared[s.share].reshape(ls)
                continue
            if s.dt == b8:
                v = rng.random(size) < 0.5
            elif red and e.op == "prod":
                slice_len = e.n if e.form == "reduce" else shape[0]
                p = min(0.25, 6.0 / slice_len)
                other = 2.0 if name == "x" else 0.5
                v = rng.choice(np.array([1.0, -1.0, other], dtype=cdt), size=size, p=[0.5 - p / 2, 0.5 - p / 2, p])
            elif red:      # max / min: a permutation (of integers around 0, scaled below 1 for the sincos program's arguments)
                v = ((rng.permutation(size) - size // 2) / (64.0 if e.progs[0][0] == "sincos" else 1.0)).astype(cdt)
            else:
                v = (rng.standard_normal(size) * 10.0 ** rng.uniform(-3, 3, size)).astype(cdt)
                if e.odt == b8:
                    v[rng.random(size) < 0.5] = 0.0
            vals[name] = v.reshape(ls)
            if s.share:
                shared[s.share] = vals[name]
        if not red:
            sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(cdt).smallest_subnormal], dtype=cdt)
            for j, p in enumerate(_marks(e)):
                if full_float:
                    vals[full_float[j % len(full_float)]].reshape(-1)[p] = sp[(j + j // len(sp)) % len(sp)]
        if plant is not None:
            pos, what = plant
            for name in PROGS[e.progs[0][0]][4]:
                assert e.leaves[name].lshape(shape) == shape, (e.id, name)
                vals[name].reshape(-1)[pos] = np.nan if what == "nan" else (BIG if e.op == "max" else -BIG)
        self.bits = bits
        self.views, self.bases = {}, {}
        for name, s in e.leaves.items():
            dt = s.dt or cdt
            if s.share and s.share in self.bases:
                base = self.bases[s.share]
            else:
                base = np.full(s.off + s.span(shape) + PAD, 1 if dt == b8 else np.nan, dtype=dt)
                self.bases[s.share or name] = base
            view = s.cut(base, shape)
            view[...] = vals[name]
            self.views[name] = view

    def _sum_values(self, bits):
        e = self.e
        vals = {}
        for k, (name, s) in enumerate(e.leaves.items()):
            if s.dt == b8:
                continue
            ls = s.lshape(e.shape)
            vals[name] = _hash_ints(int(np.prod(ls, dtype=np.int64)), bits, k + 16 * self.draw).astype(e.cdt).reshape(ls)
        rng = np.random.default_rng([zlib.crc32(e.id.encode()), 11, self.draw])
        for name, s in e.leaves.items():
            if s.dt == b8:
                vals[name] = rng.random(s.lshape(e.shape)) < 0.5
        return vals

    def _sum_fits(self, vals):
        """every value of the chain an integer that float64 holds exactly, and the magnitudes of every reduced slice sum below 2^24 / 2^53"""
        e = self.e
        wide = {n: (v if v.dtype == b8 else v.astype(f64)) for n, v in vals.items()}
        chain = np.broadcast_to(self.chain(wide, 0), e.shape)
        mass = np.abs(chain).sum(axis=None if e.form == "reduce" else 0)
        # (|x| + |y| .. in place of the operands bounds every intermediate of the program as well)
        bound = np.broadcast_to(self.chain({n: (v if v.dtype == b8 else np.abs(v) + 4.0) for n, v in wide.items()}, 0, plus=True), e.shape)
        lim = 2.0 ** 24 if e.cdt == f32 else 2.0 ** 53
        return bool(np.all(mass < lim) and np.all(np.abs(bound) < lim))

    def chain(self, views, k, plus=False):
        """program k of the entry in NumPy over `views` (plus: every subtraction an addition: a bound of the magnitudes)"""
        e = self.e
        prog, names = e.progs[k]
        o = _NP
        if plus:
            class o(_NP):      # noqa: N801
                subtract = np.add
        first = next(v for v in views.values() if v.dtype != b8)
        c = tuple(first.dtype.type(abs(x) if plus else x) for x in e.consts)
        with np.errstate(all="ignore"):
            return PROGS[prog][0](o, c, *[views[n] for n in names])

    def references(self, views=None):
        """per program: NumPy's value of the chain in the compute dtype, broadcast to the entry's shape"""
        views = views or self.views
        return [np.ascontiguousarray(np.broadcast_to(self.chain(views, k), self.e.shape)).astype(self.e.cdt, copy=False) for k in range(len(self.e.progs))]

    def reduced(self, chain):
        e = self.e
        with np.errstate(all="ignore"):
            r = getattr(np, e.op)(chain.astype(f64), axis=None if e.form == "reduce" else 0)
        return np.asarray(r).astype(e.cdt).reshape(e.red_shape)

    def insensitive(self):
        """the (leaf, axis) pairs along which a roll by one leaves every reference as it is"""
        e = self.e
        final = (lambda r: self.reduced(r)) if e.op else (lambda r: (r != 0) if e.odt == b8 else r)
        ref = [final(r) for r in self.references()]
        same, done = [], set()
        for name, s in e.leaves.items():
            if (s.share or name) in done:
                continue
            done.add(s.share or name)
            v = self.views[name]
            for ax in range(v.ndim):
                if v.shape[ax] > 1:
                    rolled = dict(self.views)
                    rolled[name] = np.roll(v, 1, axis=ax)
                    for other, so in e.leaves.items():
                        if other != name and s.share and so.share == s.share:
                            rolled[other] = rolled[name].reshape(so.lshape(e.shape))
                    new = [final(r) for r in self.references(rolled)]
                    users = [k for k, (_, names) in enumerate(e.progs) if name in names or any(e.leaves[n].share and e.leaves[n].share == s.share for n in names)]
                    if any(np.array_equal(_bits(new[k]), _bits(ref[k])) for k in users):
                        same.append((name, ax))
        return same

    # -- device side --
    def upload(self, nd):
        e = self.e
        dbases = {k: nd.asarray(b) for k, b in self.bases.items()}
        self.dviews = {name: s.dcut(dbases[s.share or name], e.shape) for name, s in e.leaves.items()}

    def make(self, nd, k=0, pending=True):
        """program k as a pending DeviceArray (pending = False: lazy mode is off, the eager chain)"""
        e = self.e
        prog, names = e.progs[k]
        r = PROGS[prog][0](nd, e.consts, *[self.dviews[n] for n in names])
        if not pending:
            assert r._expr is None and r.shape == e.shape, (e.id, prog, "should be evaluated")
            return r
        assert r._expr is not None and r._buf is None and r.shape == e.shape, (e.id, prog, "should be pending")
        n_instr, depth = PROGS[prog][3]
        assert (r._expr.n, r._expr.depth) == (n_instr, depth), (e.id, prog, r._expr.n, r._expr.depth)
        return r


def _out_base(spec, shape, dt):
    n = spec.off + spec.span(shape) + PAD
    return np.full(n, 0x5A, dtype=np.uint8).view(b8) if dt == b8 else np.full(n, SENT, dtype=dt)


def _expect(spec, shape, dt, ref):
    base = _out_base(spec, shape, dt)
    spec.cut(base, shape)[...] = ref
    return base


def _launched(lib):
    st = (C.c_int64 * 2)()
    lib.vm_jit_stats(st)
    return int(st[1])


def _counted(lib, e, leg, fn, launches=None):
    """fn() must make the entry's number of generated launches (generated leg) or none (interpreter leg; the double counts none)"""
    want = {"generated": e.launches if launches is None else launches, "interpreter": 0, "double": 0}[leg]
    l0 = _launched(lib)
    r = fn()
    assert _launched(lib) - l0 == want, f"{e.id} [{leg}]: {_launched(lib) - l0} generated launches, {want} stated"
    return r


def _shape_like(e):
    d = _capi.ArrayDesc()
    d.dtype = _capi.F32 if e.cdt == f32 else _capi.F64
    d.ndim = len(e.shape)
    d.shape[:len(e.shape)] = e.shape
    return d


def _final(e, ref):
    with np.errstate(all="ignore"):
        return (ref != 0) if e.odt == b8 else ref.astype(e.odt)


def _run_eval(nd, lib, e, leg, D):
    """evaluations and multi-output evaluations: every program against its eager twin and (where exact) NumPy, whole bases"""
    arrs = [D.make(nd, k) for k in range(len(e.progs))]
    eager = [_eager(nd, (lambda k=k: D.make(nd, k, pending=False))) for k in range(len(e.progs))]
    built = [nd._lz.build_program(a._expr, a.shape) for a in arrs]
    dob = [nd.asarray(_out_base(s, e.shape, e.odt)) for s in e.outs]
    views = [s.dcut(b, e.shape) for s, b in zip(e.outs, dob)]
    if e.form == "eval":
        _counted(lib, e, leg, lambda: lib.vm_eval(built[0][0], views[0].desc()))
    else:
        progs, outs = (_capi.VmProgram * len(arrs))(), (_capi.ArrayDesc * len(arrs))()
        for k in range(len(arrs)):
            progs[k], outs[k] = built[k][0], views[k].desc()
        _counted(lib, e, leg, lambda: lib.vm_eval_multi(progs, outs, len(arrs)))
    refs = D.references()
    for k, (prog, _) in enumerate(e.progs):
        got = dob[k].get()
        _same(got, _expect(e.outs[k], e.shape, e.odt, _final(e, eager[k])), f"{e.id} [{leg}] program {k} ({prog}) against the eager chain, whole base")
        if PROGS[prog][2]:
            _same(got, _expect(e.outs[k], e.shape, e.odt, _final(e, refs[k])), f"{e.id} [{leg}] program {k} ({prog}) against NumPy, whole base")
    del built


def _run_reduce(nd, lib, e, leg, D, what=""):
    """vm_reduce (full, axis 0) and vm_eval_reduce_cols: twice, the same bits, NumPy's reduction of the eager chain"""
    chain = _eager(nd, lambda: D.make(nd, pending=False))
    ref = D.reduced(chain)
    code, mask = CODES[e.op], (1 << len(e.shape)) - 1 if e.form == "reduce" else 1
    runs = []
    for _ in range(2):
        a = D.make(nd)
        prog, keep = nd._lz.build_program(a._expr, a.shape)
        dred = nd.asarray(_out_base(e.outs[-1], e.red_shape, e.cdt))
        rview = e.outs[-1].dcut(dred, e.red_shape)
        if e.form == "evalcols":
            dev = nd.asarray(_out_base(e.outs[0], e.shape, e.cdt))
            eview = e.outs[0].dcut(dev, e.shape)
            if leg == "interpreter":      # the one-pass form has no interpreter kernel: an error, nothing launched, nothing written
                with pytest.raises(ValueError, match="not covered by the one-pass kernel"):
                    _counted(lib, e, leg, lambda: lib.vm_eval_reduce_cols(prog, code, eview.desc(), rview.desc()))
                _same(dev.get(), _out_base(e.outs[0], e.shape, e.cdt), f"{e.id} [{leg}]{what}: a refused call wrote the evaluated output")
                _same(dred.get(), _out_base(e.outs[-1], e.red_shape, e.cdt), f"{e.id} [{leg}]{what}: a refused call wrote the reduced output")
                return
            _counted(lib, e, leg, lambda: lib.vm_eval_reduce_cols(prog, code, eview.desc(), rview.desc()))
            _same(dev.get(), _expect(e.outs[0], e.shape, e.cdt, chain), f"{e.id} [{leg}]{what}: the stored chain against the eager one, whole base")
        else:
            _counted(lib, e, leg, lambda: lib.vm_reduce(prog, code, _shape_like(e), rview.desc(), mask))
        del keep
        runs.append(dred.get())
        _same(runs[-1], _expect(e.outs[-1], e.red_shape, e.cdt, ref), f"{e.id} [{leg}]{what}: {e.op} against NumPy on the eager chain, whole base")
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])), f"{e.id} [{leg}]{what}: two runs, different bits"
    return chain


def _set_options(e, mdopt, leg):
    if leg != "double":
        mdopt("jit_min", 1)
        mdopt("jit", 1 if leg == "generated" else 0)
    for k, v in e.opts.items():
        mdopt(k, v)


def _check_exact(e, D, chain):
    """the reduction data is what the docstring says: exact in any order"""
    if e.op == "sum":
        lim = 2.0 ** 24 if e.cdt == f32 else 2.0 ** 53
        assert np.all(chain == np.rint(chain)) and np.all(np.abs(chain.astype(f64)).sum(axis=None if e.form == "reduce" else 0) < lim), e.id
    elif e.op == "prod":
        m, _ = np.frexp(np.abs(chain.astype(f64)))
        assert np.all(m == 0.5), e.id
        assert np.all(np.abs(np.log2(np.abs(chain.astype(f64)))).sum(axis=None if e.form == "reduce" else 0) < 100), e.id


def _check_entry(case, lib, mdopt, leg):
    from minidiff_amd import ndarray as nd
    e = BY_ID[case]
    _set_options(e, mdopt, leg)
    prev = nd.set_lazy(True)
    try:
        plants = [None] + [(p, w) for p in e.positions for w in ("ext", "nan")]
        for plant in plants:
            D = Data(e, plant)
            if leg == "double" and plant is None:
                same = D.insensitive()
                assert not same, (e.id, f"(leaf, axis) {same}: rolled by one, same reference")
            D.upload(nd)
            if e.form in ("eval", "multi"):
                _run_eval(nd, lib, e, leg, D)
                continue
            chain = _run_reduce(nd, lib, e, leg, D, "" if plant is None else f" {plant}")
            if leg == "double":
                _check_exact(e, D, chain)
                if plant is not None:      # the planted position IS the extreme / the NaN of its slice
                    flat = chain.reshape(-1)
                    if plant[1] == "nan":
                        assert np.isnan(flat[plant[0]]) and np.isnan(flat).sum() == 1, (e.id, plant)
                    else:
                        assert (np.argmax(flat) if e.op == "max" else np.argmin(flat)) == plant[0], (e.id, plant)
    finally:
        nd.set_lazy(prev)


BOTH = [e.id for e in TABLE if not e.no_double]
ON_GPU = [e.id for e in TABLE]


@pytest.mark.parametrize("case", BOTH)
def test_paths(lib, on_gpu, mdopt, case):
    """CPU double: the data, the references, the position-sensitivity check, the C-ABI calls"""
    if on_gpu:
        pytest.skip("other twin")
    _check_entry(case, lib, mdopt, "double")


@gpu
@pytest.mark.parametrize("leg", ["generated", "interpreter"])
@pytest.mark.parametrize("case", ON_GPU)
def test_paths_gpu(lib, on_gpu, mdopt, case, leg):
    assert on_gpu and lib.target == "hip:gfx950"
    _check_entry(case, lib, mdopt, leg)


# ---------------------------------------------------------------------------------------------------------------- through nd.*
PUBLIC = [e.id for e in TABLE if e.public]


def _check_public(case, lib, mdopt, leg):
    """the entry through nd.* with lazy mode on: FUSION_STATS moves, the operand of a reduction stays pending, the same bits"""
    from minidiff_amd import ndarray as nd
    e = BY_ID[case]
    _set_options(e, mdopt, leg)
    prev = nd.set_lazy(True)
    try:
        D = Data(e)
        D.upload(nd)
        S = nd.FUSION_STATS
        eager = [_eager(nd, (lambda k=k: D.make(nd, k, pending=False))) for k in range(len(e.progs))]
        if e.form == "eval":
            a = D.make(nd)
            s0 = S["vm_eval"]
            got = _counted(lib, e, leg, a.get)
            assert S["vm_eval"] - s0 == 1, e.id
            _same(got, eager[0], f"{e.id} [{leg}] through nd.*")
        elif e.form == "multi":
            arrs = [D.make(nd, k) for k in range(len(e.progs))]
            s0 = S["vm_eval_multi"]
            _counted(lib, e, leg, lambda: nd.materialize_many(arrs))
            assert S["vm_eval_multi"] - s0 == 1 and all(a._buf is not None for a in arrs), e.id
            for k, a in enumerate(arrs):
                _same(a.get(), eager[k], f"{e.id} [{leg}] program {k} through nd.materialize_many")
        else:
            a = D.make(nd)
            s0 = S["vm_reduce"]
            r = _counted(lib, e, leg, lambda: getattr(nd, e.op)(a, axis=None if e.form == "reduce" else 0))
            assert S["vm_reduce"] - s0 == 1, (e.id, "not fused")
            assert a._buf is None and a._expr is not None, (e.id, "the reduction materialised its operand")
            _same(np.asarray(r.get()).reshape(e.red_shape), D.reduced(eager[0]), f"{e.id} [{leg}] {e.op} through nd.*")
    finally:
        nd.set_lazy(prev)


@pytest.mark.parametrize("case", PUBLIC)
def test_public(lib, on_gpu, mdopt, case):
    if on_gpu:
        pytest.skip("other twin")
    _check_public(case, lib, mdopt, "double")


@gpu
@pytest.mark.parametrize("leg", ["generated", "interpreter"])
@pytest.mark.parametrize("case", PUBLIC)
def test_public_gpu(lib, on_gpu, mdopt, case, leg):
    assert on_gpu and lib.target == "hip:gfx950"
    _check_public(case, lib, mdopt, leg)


def _check_owed(lib, mdopt, leg):
    """sum(where(m, x, y), axis=0) of a (512, 1024) chain is OWED until the chain is needed in memory; then one call evaluates and
    reduces (generated: the strips kernel with store, one launch; otherwise the refusal and two passes)"""
    from minidiff_amd import ndarray as nd
    if leg != "double":
        mdopt("jit_min", 1)
        mdopt("jit", 1 if leg == "generated" else 0)
    e = Entry("owed-512x1024", "SWEEP with store through DeviceArray._materialize", "evalcols", (512, 1024), [("where", ["m", "x", "y"])],
              {"m": V(dt=b8), "x": V(), "y": V()}, [V(), V()], op="sum")
    prev = nd.set_lazy(True)
    try:
        D = Data(e)
        D.upload(nd)
        S = nd.FUSION_STATS
        chain = _eager(nd, lambda: D.make(nd, pending=False))
        a = D.make(nd)
        d0 = S["deferred_cols"]
        r = nd.sum(a, axis=0)
        assert S["deferred_cols"] - d0 == 1 and a._buf is None, "the column sum was not owed"
        stat = "vm_eval" if leg == "interpreter" else "vm_eval_reduce_cols"
        s0, l0 = S[stat], _launched(lib)
        got = a.get()
        assert S[stat] - s0 == 1, (leg, stat)
        assert _launched(lib) - l0 == (1 if leg == "generated" else 0), leg
        _same(got, chain, f"owed column sum [{leg}]: the evaluated chain")
        _same(r.get().reshape(1, 1024), D.reduced(chain), f"owed column sum [{leg}]: the sums")
    finally:
        nd.set_lazy(prev)


def test_owed_column_sum(lib, on_gpu, mdopt):
    if on_gpu:
        pytest.skip("other twin")
    _check_owed(lib, mdopt, "double")


@gpu
@pytest.mark.parametrize("leg", ["generated", "interpreter"])
def test_owed_column_sum_gpu(lib, on_gpu, mdopt, leg):
    assert on_gpu and lib.target == "hip:gfx950"
    _check_owed(lib, mdopt, leg)


# ---------------------------------------------------------------------------------------------------------------------- refusals
# id -> (shape, form, what is off, the C-ABI's message)
REFUSALS = {
    "refuse-evalcols-n_red-below-512": ((511, 260), "evalcols", None, "not covered by the one-pass kernel"),
    "refuse-evalcols-n_out-odd": ((512, 258), "evalcols", None, "geometry not supported"),
    "refuse-evalcols-out-misaligned": ((512, 260), "evalcols", "eval", "unaligned output"),
    "refuse-evalcols-red-misaligned": ((512, 260), "evalcols", "red", "unaligned output"),
    "refuse-cols-n_out-odd": ((512, 258), "cols", None, "vm_reduce"),
    "refuse-cols-out-misaligned": ((512, 260), "cols", "red", "unaligned output"),
    "refuse-reduce-out-misaligned": ((4 * 769 + 3,), "reduce", "red", "unaligned output"),
    "refuse-reduce-one-element": ((1,), "reduce", None, "geometry not supported"),
}


def _refusal_entry(case):
    shape, form, off, msg = REFUSALS[case]
    outs = [V(off=PAD + 1 if off == "eval" else PAD), V(off=PAD + 1 if off == "red" else PAD)]
    return Entry(case, "a refusal of the launcher", form, shape, [("where", ["m", "x", "y"])], {"m": V(dt=b8), "x": V(), "y": V()},
                 outs if form != "reduce" else outs[1:], op="sum"), msg


@gpu
@pytest.mark.parametrize("leg", ["generated", "interpreter"])
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_gpu(lib, on_gpu, mdopt, case, leg):
    """the refusals the launchers document: an error at the C-ABI, no generated launch, nothing written"""
    from minidiff_amd import ndarray as nd
    assert on_gpu and lib.target == "hip:gfx950"
    e, msg = _refusal_entry(case)
    _set_options(e, mdopt, leg)
    prev = nd.set_lazy(True)
    try:
        D = Data(e)
        D.upload(nd)
        a = D.make(nd)
        prog, keep = nd._lz.build_program(a._expr, a.shape)
        dred = nd.asarray(_out_base(e.outs[-1], e.red_shape, e.cdt))
        rview = e.outs[-1].dcut(dred, e.red_shape)
        l0 = _launched(lib)
        with pytest.raises(ValueError, match=msg):
            if e.form == "evalcols":
                dev = nd.asarray(_out_base(e.outs[0], e.shape, e.cdt))
                lib.vm_eval_reduce_cols(prog, _capi.R_SUM, e.outs[0].dcut(dev, e.shape).desc(), rview.desc())
            else:
                lib.vm_reduce(prog, _capi.R_SUM, _shape_like(e), rview.desc(), 1 if e.form == "cols" else (1 << len(e.shape)) - 1)
        assert _launched(lib) == l0, case
        _same(dred.get(), _out_base(e.outs[-1], e.red_shape, e.cdt), f"{case}: a refused call wrote its output")
    finally:
        nd.set_lazy(prev)


def _check_refused_public(case, lib, mdopt, leg):
    """.. and the same shapes through nd.*: the eager values, whichever route ndarray.py takes"""
    from minidiff_amd import ndarray as nd
    e, _ = _refusal_entry(case)
    _set_options(e, mdopt, leg)
    prev = nd.set_lazy(True)
    try:
        D = Data(e)
        D.upload(nd)
        chain = _eager(nd, lambda: D.make(nd, pending=False))
        a = D.make(nd)
        r = nd.sum(a, axis=None if e.form == "reduce" else 0)
        _same(np.asarray(r.get()).reshape(e.red_shape), D.reduced(chain), f"{case} [{leg}] through nd.*: the sums")
        _same(a.get(), chain, f"{case} [{leg}] through nd.*: the chain")
    finally:
        nd.set_lazy(prev)


_REFUSED_SHAPES = ["refuse-evalcols-n_red-below-512", "refuse-evalcols-n_out-odd", "refuse-reduce-one-element"]


@pytest.mark.parametrize("case", _REFUSED_SHAPES)
def test_refused_shapes_public(lib, on_gpu, mdopt, case):
    if on_gpu:
        pytest.skip("other twin")
    _check_refused_public(case, lib, mdopt, "double")


@gpu
@pytest.mark.parametrize("leg", ["generated", "interpreter"])
@pytest.mark.parametrize("case", _REFUSED_SHAPES)
def test_refused_shapes_public_gpu(lib, on_gpu, mdopt, case, leg):
    assert on_gpu and lib.target == "hip:gfx950"
    _check_refused_public(case, lib, mdopt, leg)


# --------------------------------------------------------------------------------------------------------------------- the table
def test_table_is_complete():
    """every form, branch and program the module docstring derives has an entry, and the derived geometry is what the ids say"""
    text = " ".join(e.reaches for e in TABLE)
    for name in ("k_vm_eval_fast", "k_fused_eval*", "k_fused_evalb", "k_fused_evalh", "k_vm_eval_generic", "k_vm_reduce_all", "k_fused_redall", "md_ticket_last2",
                 "k_vm_reduce_cols", "k_fused_redcols", "second pass", "k_fused_sweepcols", "k_fused_evalcols", "k_fused_eval2", "k_fused_eval3", "k_fused_eval4",
                 "LM_ROWB", "LM_CONST", "uncollapse_2d", "padded row pitch", "md_fold_partials", "declined"):
        assert name in text, name
    assert all(e.reaches and e.shape for e in TABLE)
    used = {p for e in TABLE for p, _ in e.progs}
    assert used == set(PROGS), set(PROGS) - used
    for form in ("eval", "reduce", "cols", "evalcols"):      # per form: every program, both dtypes, the four leaf modes in one entry
        es = [e for e in TABLE if e.form == form and (form != "eval" or e.launches)]
        assert {f32, f64} <= {e.cdt for e in es}, form
        assert any(e.progs[0][0] == "d4" and [s.keep for s in e.leaves.values()] == [None, ROW, COL, ONE] for e in es), form
        want = {"two", "where", "sincos", "d4", "eight", "long44"} - ({"sincos", "eight", "long44"} if form == "evalcols" else set())
        assert want <= {e.progs[0][0] for e in es}, (form, want - {e.progs[0][0] for e in es})
    # (rows, inner) evaluation: the group counts around one and two grid strides, every tail, the four (dq, dr) classes
    nvs = {(e.n // 4, e.n % 4) for e in TABLE if e.form == "eval" and len(e.shape) == 1 and e.opts == MB3 and e.launches}
    assert {0, 1, 767, 768, 769, 1535, 1536, 1537, 2305, 3073} <= {nv for nv, _ in nvs}
    assert {(nv, t) for nv in (769, 1537) for t in range(4)} <= nvs and {(0, 2), (0, 3)} <= nvs
    dqr = {divmod(T, e.shape[1] // 4) for e in TABLE if e.form == "eval" and len(e.shape) == 2 and e.opts == MB3 and e.launches}
    assert any(q and r for q, r in dqr) and any(q and not r for q, r in dqr) and any(not q and r for q, r in dqr)
    assert all(e.shape[0] * (e.shape[1] // 4) > T for e in TABLE if e.id.startswith("eval-2d-"))
    # full reduction: both ticket protocols, shards of different counts
    caps = {e.opts["max_blocks"] for e in TABLE if e.id.startswith("redall-cap")}
    assert caps == {1, 3, 63, 64, 65, 97} and all(e.n // 4 > 256 * e.opts["max_blocks"] for e in TABLE if e.id.startswith("redall-cap"))
    # tiled column reduction: direct writes, a second pass, a short last chunk, chunk2 > splits and chunk2 == splits
    sp = {e.shape: _splits(*e.shape) for e in TABLE if e.id.startswith("cols-")}
    assert {1, 4, 31, 32, 33, 63, 64, 65, 100, 511, 512, 513, 2000} <= {s[0] for s in sp} and {4, 252, 256, 260, 516, 1028} <= {s[1] for s in sp}
    assert any(s == 1 for s, _ in sp.values()) and any(s > 1 and shape[0] % c for shape, (s, c) in sp.items())
    assert any(s > 1 and -(-s // 16) * 16 > s for s, _ in sp.values()) and any(s > 1 and s % 16 == 0 for s, _ in sp.values())
    assert _splits(65, 260) == (2, 48) and _splits(100, 260) == (3, 48) and _splits(511, 260) == (11, 48) and _splits(2000, 260) == (42, 48)
    # strips: band counts, rows per trip, every shape of the pipeline, ragged strips
    nbts, nbs, rus, tails = set(), set(), set(), set()
    for e in TABLE:
        if e.id.startswith("sweep-"):
            sizes = [1 if n == "m" else e.cdt.itemsize for n, s in e.leaves.items() if s.keep is None]
            _, NB, RU, nrw = _sweep_reach(e.shape[0], e.shape[1], e.opts.get("sweep_nb", 0), e.opts.get("sweep_ru", 0), sizes)
            assert e.shape[0] >= 512 and e.shape[1] % 4 == 0 and min(nrw) >= RU, e.id
            nbs.add(NB)
            rus.add(RU)
            nbts |= {r // RU for r in nrw}
            tails |= {r % RU for r in nrw}
            assert e.id.endswith(("eight", "long44", "sincos")) or BY_ID["evalcols-" + e.id[6:]].shape == e.shape, e.id
    assert {1, 2, 3, 4} <= nbts and {1, 2, 3, 64} <= nbs and {1, 2, 8} <= rus and {0, 1} <= tails, (nbts, nbs, rus, tails)
    assert {4, 252, 256, 260, 516} <= {e.shape[1] for e in TABLE if e.id.startswith("sweep-")}
    # multi-output: 2, 3, 4 programs, every tail, immediates in every program, the declined cases
    assert {2, 3, 4} <= {len(e.progs) for e in TABLE if e.form == "multi"}
    assert {0, 1, 2, 3} <= {e.n % 4 for e in TABLE if e.form == "multi" and len(e.shape) == 1}
    assert sum(1 for e in TABLE if e.id.startswith("multi-declined")) == 3
    assert len(PUBLIC) >= 12 and len(TABLE) >= 150


def test_programs_are_what_the_docstring_says(lib):
    """instruction counts and stack depths as lazy.py builds them; long44 is the longest program it builds"""
    from minidiff_amd import lazy, ndarray as nd
    assert PROGS["long44"][3][0] == lazy.MAX_INSTR and PROGS["d4"][3][1] == lazy.MAX_DEPTH and len(PROGS["eight"][1]) == lazy.MAX_LEAVES
    prev = nd.set_lazy(True)
    try:
        for e in (BY_ID["gen-long44"], BY_ID["gen-d4-modes"], BY_ID["gen-eight"], BY_ID["gen-sincos"], BY_ID["multi-3-2d"]):
            D = Data(e)
            D.upload(nd)
            for k in range(len(e.progs)):
                a = D.make(nd, k)      # (asserts n and depth)
                prog, keep = nd._lz.build_program(a._expr, a.shape)
                assert prog.n_instr == PROGS[e.progs[k][0]][3][0] and prog.n_leaves == len(set(e.progs[k][1]))
    finally:
        nd.set_lazy(prev)
