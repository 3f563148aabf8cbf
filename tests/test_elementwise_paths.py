"""Every launch form of the elementwise kernels, wide and narrow (csrc/elementwise.hip: k_ew_fast, k_ew_axes, k_unary_tr, the three
generic kernels, k_arange, k_convert; csrc/narrow.hip: k_nw_unary, k_nw_binary, k_nw_binary_axes, the three generic kernels) against
NumPy, bit for bit.

The centre is TABLE: what an entry reaches (kernel, template form, branch), the operands (each a view cut from a larger base), the
output view, the ops, the dtypes, the options. There is no hook that reports which kernel ran: every shape is derived from the
launchers' predicates, and the `reaches` column is confirmed by a kernel trace of the gpu half (profiles/README.md:
elementwise_paths_kernel_stats.csv).

Where the numbers come from:
  MD_BLOCK 256, MD_NUM_CUS 256   md_grid_for(work, 256, cap) = min(ceil(work / 256), cap) blocks; the default cap is 8 per CU = 2048
                                 blocks (one grid trip of the generic kernels and of k_arange: 2048 * 256 = 524288 elements).
  launch_fast                    vectors of 4 elements; the cap is Body::kBlocksPerCU per CU — 4 for the cheap unary functors and
                                 every binary body, 8 for `where`: a trip is 262144 / 524288 vectors — unless option max_blocks is
                                 set: max_blocks = 3 makes the stride 768 vectors. (dq, dr) = divmod(stride, nv) with nv vectors per
                                 row: nv 5 / 7 give dq and dr non-zero, nv 768 gives dr = 0, nv 1000 gives dq = 0 and the wrap of
                                 `cv >= nv`. 1-D: the n % 4 elements behind the last vector go to lanes 0 .. 2 (`tail`).
  MD_EW_UNROLL 2                 the VEC / SCAL forms take two vectors per lane and trip while v + stride < total, then one: with
                                 stride 768, totals 767 / 768 (no main trip, last lane idle / busy), 769 (lane 0 alone has a main
                                 trip), 1535 / 1536 / 1537 (every lane a main trip; 1537: lane 0 a tail trip as well), 2305, 3073
                                 (main loop, then the one-vector loop). MD_EW_UNROLL_NT 1 (option nt = 1) and the FLEX forms (every
                                 integer and bool binary loop; column-broadcast operands) have the one-vector loop only.
  fast_geom / fast_operand       output unit-stride (2-D: dense rows, inner % 4 == 0) and on its vector alignment (min(16, 4 *
                                 element size)); every array operand of the loop's storage dtype with inner stride 0 or 1, a
                                 unit-stride one aligned and (2-D) with row stride % 4 == 0. One entry per refusal.
  md_ld_stream / md_st_stream    the non-temporal branch exists for 16-byte vectors only: float32 / int32. float64 / int64 vectors
                                 are 32 B and bool's are 4 B: nt = 1 picks the NT template (one-vector loop) with plain accesses.
  axes_geom                      3 or 4 collapsed axes, total >= 2^16, inner % 4 == 0, output dense and aligned, every array operand
                                 of the dtype the kernel reads, inner stride 0 or 1, a unit-stride one aligned with outer strides
                                 % 4 == 0. (5, 37, 356) = 65860 and (3, 5, 37, 120) = 66600 are non-powers of two in every extent;
                                 (5, 37, 352) = 65120 is the refusal below 65536.
  tr_geom                        total >= 2^14, R >= 32, Cn >= 32, output dense (B, R, Cn), source unit-stride along R with column
                                 stride >= R: 64 x 64 tiles; (130, 127) has partial tiles on both edges, (129, 127) = 16383.
  nw_contiguous / nw_grid        one storage-only dtype, everything dense and on 16 B; E = 16 / element size elements per vector;
                                 the cap is explicit (max_blocks does not reach it): 4 blocks per CU for VEC/VEC (stride 262144
                                 vectors), 8 for the unary and scalar forms (524288). md_grid_for(nv + 1) grows with the work, so
                                 the two-in-flight loop (`i + gs < nv`) first runs at nv = stride + 1: 262145, 2 * 262144 + 5,
                                 3 * 262144 + 1; 524289, 2 * 524288 + 5. NT: one vector in flight.
  binary_axes (narrow)           2 - 4 collapsed axes, total >= 2^14, inner % E == 0, output dense on sizeof(So) * E bytes, operands
                                 of the one storage dtype, unit-stride ones on 16 B with strides % E == 0. (34, 480) = 16320 refuses.
  k_convert                      the carrier follows the SOURCE: int64 (bool, signed), uint64 (unsigned), double (floats).

Not reachable at test size (no entry pretends otherwise): the 64-bit branch of k_ew_axes (2^31 vectors and more) and the 64-bit
division of md_ew_drive (2^32 vectors per row, or a lane index beyond 2^32).

Data — every comparison is `==` on raw bits (arrays viewed as unsigned integers: NaN payloads and -0.0 count), no tolerance anywhere:
  integers   an element counter times an odd constant, reinterpreted in the dtype: full range, wrap-around must be NumPy's; divisors
             of floor_divide / mod: zeros replaced.
  floats     normals * 10^uniform(-3, 3) (float16: 10^uniform(-1, 1)), with NaN, +-inf, +-0.0 and subnormals planted at element 0,
             the last element of the first vector, both sides of the vector boundaries next to the tail, every tail element, both
             sides of every grid-trip boundary; N-D: the first and last vector of the first, a middle and the last row (and rows /
             columns 63 and 64: the corners of k_unary_tr's partial tiles). At one logical position at most ONE operand of the
             output's shape holds a special (so no inf - inf, 0 * inf: the sign of a NaN an operation CREATES is the platform's),
             broadcast operands hold NaN and subnormals only, a subtrahend holds no NaN (the sign a propagated NaN takes through a
             negated operand is the platform's), the divisor of floor_divide / mod holds none and their dividend no inf. float16
             results are NumPy's own float16 loops'.
  per op     equal / not_equal draw from an alphabet of four values; the logical ops and logical_not get half zeros; isnan gets
             random NaNs: otherwise their reference is constant and says nothing about position.
  padding    every operand is a view inside a larger base that holds a sentinel (NaN for floats, a fixed pattern for integers), the
             output a view inside a sentinel base of this module's own; the WHOLE output base is compared: a store past the end
             fails, an unwritten output fails, a read outside a view poisons a float result.
  casts      values in range of the destination; int64 -> float32 around 2^24 + 1, int64 -> float64 around 2^53 + 1, float64 ->
             float32 ties / overflow to inf / subnormal results, anything -> bool with 0.5, -0.0, NaN and a subnormal, a few float16
             ties (1 + 2^-11 ..) on every path that writes float16.
  arange     start and step dyadic, every value exactly representable: the reference is np.arange.

Position sensitivity (CPU twin, _check_sensitive): for every entry, dtype and op, rolling any array operand by one along any of its
axes longer than 1 changes the reference — a misplaced vector or row cannot pass. (Host scalars and one-element device operands have
nothing to roll.)

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound) — it proves data and references right — and gpu-marked
on the product library; test_paths goes through the C-ABI the way ndarray.py does at its end (DeviceArray descriptors + lib.unary /
binary / where / convert / fill / arange), test_public runs the same entries through nd.* with lazy mode off. Not run on both twins:
fast-default-grid-second-trip (gpu only: 2 * 2^20 + 7 elements say nothing on the double, which has one loop).

Found with it (both fail on the library as it was before): nw-vec-scal-* / nw-scal-vec-*, float16 multiply — the scalar tail of
k_nw_binary rounded the float32 product to float16 as fma(x, y, +0): -0.0 * y came out +0.0 behind the last vector; nw-unary-*, float16
sqrt — a NaN came out of the stream kernel with its sign bit set, out of every other path without (USqrt now hands a NaN on as it is)."""
import itertools

import numpy as np
import pytest

from minidiff_amd import _capi
from minidiff_amd import ndarray as nd

f16, f32, f64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
i8, i16, i32, i64 = np.dtype(np.int8), np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.int64)
u8, u16, u32, u64 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)
b8 = np.dtype(np.bool_)
W5 = (f32, f64, i32, i64, b8)                # the dtypes the wide kernels compute in
N7 = (i8, i16, u8, u16, u32, u64, f16)       # storage-only
ALL12 = W5 + N7
BY_SIZE = (i8, f16, u32, u64)                # one storage-only dtype per element size
PAD = 16                                     # sentinel elements before and after every view (a multiple of 16 B for every size)
MD_BLOCK, MD_NUM_CUS = 256, 256
FAST_TRIP = MD_NUM_CUS * 4 * MD_BLOCK        # vectors per grid trip of k_ew_fast at 4 blocks per CU
NW_TRIP_VV, NW_TRIP = MD_NUM_CUS * 4 * MD_BLOCK, MD_NUM_CUS * 8 * MD_BLOCK      # .. of k_nw_binary VEC/VEC; of the other stream forms
GRID_TRIP = 2048 * MD_BLOCK                  # elements per grid trip of the generic kernels and k_arange

U_CODE = {"copy": _capi.U_COPY, "negative": _capi.U_NEG, "absolute": _capi.U_ABS, "sign": _capi.U_SIGN, "floor": _capi.U_FLOOR, "ceil": _capi.U_CEIL,
          "sqrt": _capi.U_SQRT, "logical_not": _capi.U_LOGICAL_NOT, "invert": _capi.U_INVERT, "isnan": _capi.U_ISNAN}
B_CODE = {"add": _capi.B_ADD, "subtract": _capi.B_SUB, "multiply": _capi.B_MUL, "true_divide": _capi.B_TRUE_DIV, "floor_divide": _capi.B_FLOOR_DIV,
          "mod": _capi.B_MOD, "maximum": _capi.B_MAXIMUM, "minimum": _capi.B_MINIMUM, "equal": _capi.B_EQ, "not_equal": _capi.B_NE, "less": _capi.B_LT,
          "less_equal": _capi.B_LE, "greater": _capi.B_GT, "greater_equal": _capi.B_GE, "logical_and": _capi.B_LAND, "logical_or": _capi.B_LOR,
          "logical_xor": _capi.B_LXOR}
CMP = ("equal", "not_equal", "less", "less_equal", "greater", "greater_equal")
LOGICAL = ("logical_and", "logical_or", "logical_xor")
U_ALL = tuple(U_CODE)
B_ALL = tuple(B_CODE)
U_GEOM = ("negative", "isnan", "invert")     # floats: negative + isnan (bool output, 4-byte vectors); integers: negative + invert; bool: invert
B_GEOM = ("add", "less")                     # output of the loop dtype; bool output


def _np_fn(op):
    return np.remainder if op == "mod" else getattr(np, op)


def _valid(op, dt):
    """The ops NumPy and the library both define for one operand dtype (mixed-dtype entries name their ops themselves)."""
    if dt.kind == "f":
        return op != "invert"
    if dt == b8:
        return op in ("copy", "logical_not", "invert", "add", "multiply", "maximum", "minimum") + CMP + LOGICAL
    return op not in ("floor", "ceil", "sqrt", "isnan", "true_divide")


class A:
    """An array operand (or the output): `shape` dense inside a 1-D sentinel base from element `off`, then `cut`. `shape` may be a
    function of E = 16 / element size. dt: the operand's dtype when it is not the entry's."""

    def __init__(self, shape, off=PAD, cut=None, dt=None):
        self.shape, self.off, self.cut, self.dt = shape, off, cut, dt

    def dense_shape(self, E):
        return tuple(self.shape(E)) if callable(self.shape) else tuple(self.shape)

    def base_len(self, E):
        return int(np.prod(self.dense_shape(E), dtype=np.int64)) + 2 * PAD + 2

    def view(self, base, E):
        shape = self.dense_shape(E)
        n = int(np.prod(shape, dtype=np.int64))
        v = base[self.off:self.off + n].reshape(shape)
        return v if self.cut is None else self.cut(v)


class K:
    """A host scalar operand (a scalar descriptor): the dtype's standard value (`second`: its other one), or `value`."""

    def __init__(self, value=None, second=False, dt=None):
        self.value, self.second, self.dt = value, second, dt

    def get(self, dt, op=None, k=0):
        if self.value is not None:
            return self.value
        if dt == b8 and op in CMP[2:]:            # (a bool against a constant: two of the four orderings are constant, on either side)
            return (op in ("less", "greater_equal")) == (k == 1)
        if op == "logical_or" or (dt == b8 and op in ("add", "maximum")):      # (with a true scalar the answer is true everywhere)
            return 0.0 if dt.kind == "f" else False if dt == b8 else 0
        if dt.kind == "f":
            return -0.25 if self.second else 1.5
        if dt == b8:
            return not self.second
        return 7 if self.second else (3 if dt.kind == "u" else -3)


class Entry:
    def __init__(self, id, reaches, kind, ins, out, ops, dtypes, nt=False, max_blocks=None, gpu_only=False, trip=FAST_TRIP, start_step=None):
        self.id, self.reaches, self.kind, self.ins, self.out, self.ops, self.dtypes = id, reaches, kind, tuple(ins), out, tuple(ops), tuple(dtypes)
        self.nt, self.max_blocks, self.gpu_only, self.trip, self.start_step = nt, max_blocks, gpu_only, trip, start_step


TABLE = []


def _e(id, reaches, kind, ins, out, ops, dtypes, **k):
    TABLE.append(Entry(id, reaches, kind, ins, out, ops, dtypes, **k))


def _ubw(id, reaches, mk, out, dtypes=W5, kinds="ubw", uops=U_GEOM, bops=B_GEOM, **k):
    """One geometry, three arities: mk(kind) -> the operands."""
    if "u" in kinds:
        _e(id + "/u", reaches, "unary", mk("unary"), out, uops, dtypes, **k)
    if "b" in kinds:
        _e(id + "/b", reaches, "binary", mk("binary"), out, bops, dtypes, **k)
    if "w" in kinds:
        _e(id + "/w", reaches, "where", mk("where"), out, ("where",), dtypes, **k)


def _same(spec_of):
    """Operands that all have one geometry (the mask of `where` in bool)."""
    def mk(kind):
        if kind == "unary":
            return [spec_of(None)]
        if kind == "binary":
            return [spec_of(None), spec_of(None)]
        return [spec_of(b8), spec_of(None), spec_of(None)]
    return mk


# ---- k_ew_fast: geometry ---------------------------------------------------------------------------------------------------------
for n in (0, 1, 2, 3, 4, 5, 6, 7, 1200, 1201, 1202, 1203):
    what = {0: "nothing is launched", 1: "one element collapses to 0 axes: the generic kernels"}.get(n, f"k_ew_fast 1-D: {n // 4} vectors + a tail of {n % 4}")
    _ubw(f"fast-1d-{n}", what, _same(lambda dt, n=n: A((n,), dt=dt)), A((n,)), kinds="ubw" if n in (3, 5, 1203) else "ub")
_ubw("fast-2d-dense", "k_ew_fast 2-D: dense output (37, 24), inner % 4 == 0; inputs with a row pitch of 32 keep the space 2-D",
     _same(lambda dt: A((37, 32), cut=lambda a: a[:, :24], dt=dt)), A((37, 24)))
for nv in (767, 768, 769, 1535, 1536, 1537, 2305, 3073):
    n = 4 * nv + nv % 4
    _ubw(f"fast-mb3-nv{nv}", f"k_ew_fast 1-D under max_blocks = 3 (stride 768 vectors): {nv} vectors + a tail of {nv % 4}",
         _same(lambda dt, n=n: A((n,), dt=dt)), A((n,)), max_blocks=3, nt=True, trip=768)
for nv, rows in ((5, 463), (7, 331), (768, 4), (1000, 3)):
    C = 4 * nv

    def mk(kind, rows=rows, C=C):
        pitched = A((rows, C + 8), cut=lambda a, C=C: a[:, :C])                # row stride C + 8, % 4 == 0: stays 2-D
        if kind == "unary":
            return [pitched]
        if kind == "binary":
            return [A((rows, C)), A((C,))]                                      # a row-broadcast operand (os = 0, is = 1): VEC/VEC
        return [A((rows, C), dt=b8), A((C,)), K()]                              # where: VEC cond, VEC (row-broadcast), SCAL
    _ubw(f"fast-mb3-2d-nv{nv}", f"k_ew_fast 2-D under max_blocks = 3: {rows} rows of {nv} vectors ({rows * nv} vectors), (dq, dr) = divmod(768, {nv})",
         mk, A((rows, C)), max_blocks=3, nt=True, trip=768)
_ubw("fast-default-grid-second-trip", "k_ew_fast at the default grid (4 blocks per CU, stride 262144 vectors): 2 * 2^20 + 7 float32 elements, a second trip",
     _same(lambda dt: A((2 * (1 << 20) + 7,), dt=dt)), A((2 * (1 << 20) + 7,)), dtypes=(f32,), kinds="ub", uops=("negative",), bops=("add",), gpu_only=True)

# refusals of the fast path, each at a shape the fast path takes when the reason is absent
_ubw("fast-refuse-out-off", "generic kernels: the output starts at element 1, off its vector alignment", _same(lambda dt: A((1203,), dt=dt)), A((1203,), off=PAD + 1))
_ubw("fast-refuse-in-off", "generic kernels: a unit-stride operand starts at element 1", _same(lambda dt: A((1203,), off=PAD + 1, dt=dt)), A((1203,)))
_ubw("fast-refuse-row-stride", "generic kernels: 2-D, an operand's row stride 30, % 4 != 0", _same(lambda dt: A((37, 30), cut=lambda a: a[:, :24], dt=dt)), A((37, 24)))
_ubw("fast-refuse-inner", "generic kernels: 2-D, inner 26, % 4 != 0", _same(lambda dt: A((37, 32), cut=lambda a: a[:, :26], dt=dt)), A((37, 26)))
_ubw("fast-refuse-inner-stride-2", "generic kernels: inner stride 2", _same(lambda dt: A((2406,), cut=lambda a: a[::2], dt=dt)), A((1203,)))
_ubw("fast-refuse-out-pitch", "generic kernels: 2-D, the output's rows are not dense (pitch 32)", _same(lambda dt: A((37, 24), dt=dt)),
     A((37, 32), cut=lambda a: a[:, :24]))

# ---- k_ew_fast: forms ------------------------------------------------------------------------------------------------------------
N1 = 1203
_e("fast-unary-vec", "k_ew_fast<UnaryBody<.., OM_VEC, NT>>: every unary op", "unary", [A((N1,))], A((N1,)), U_ALL, W5, nt=True)
_e("fast-unary-scal-device", "k_ew_fast<UnaryBody<.., OM_SCAL, NT>>: a stride-0 view of one device element", "unary", [A((1,))], A((N1,)), U_ALL, W5, nt=True)
_e("fast-unary-scal-host-copy", "k_ew_fast<UnaryBody<UCopy, .., OM_SCAL, NT>>: U_COPY of a host scalar", "unary", [K()], A((N1,)), ("copy",), W5, nt=True)
_e("fast-fill", "mdhip_fill: k_ew_fast<UnaryBody<UCopy, .., OM_SCAL, NT>>, 1-D and (dense rows) collapsed", "fill", [K()], A((N1,)), ("fill",), W5, nt=True)
_e("fast-unary-flex", "k_ew_fast<UnaryBody<.., OM_FLEX, false>, 1>: a (37, 1) column broadcast to (37, 24)", "unary", [A((37, 1))], A((37, 24)), U_ALL, W5, nt=True)
_e("fast-binary-vec-vec", "k_ew_fast<BinaryBody<.., OM_VEC, OM_VEC, NT>> (integers, bool: OM_FLEX, OM_FLEX, U = 1): every binary op", "binary",
   [A((N1,)), A((N1,))], A((N1,)), B_ALL, W5, nt=True)
_e("fast-binary-vec-scal", "BinaryBody<.., OM_VEC, OM_SCAL, NT>: a host scalar on the right", "binary", [A((N1,)), K()], A((N1,)), B_ALL, W5, nt=True)
_e("fast-binary-scal-vec", "BinaryBody<.., OM_SCAL, OM_VEC, NT>: a host scalar on the left", "binary", [K(), A((N1,))], A((N1,)), B_ALL, W5, nt=True)
_e("fast-binary-vec-scal-device", "BinaryBody<.., OM_VEC, OM_SCAL, NT>: one device element on the right (read in the prologue)", "binary", [A((N1,)), A((1,))], A((N1,)),
   ("add", "subtract", "floor_divide", "less", "logical_and"), W5, nt=True)
_e("fast-binary-scal-vec-device", "BinaryBody<.., OM_SCAL, OM_VEC, NT>: one device element on the left", "binary", [A((1,)), A((N1,))], A((N1,)),
   ("add", "subtract", "floor_divide", "less", "logical_and"), W5, nt=True)
_e("fast-binary-flex-col", "BinaryBody<.., OM_FLEX, OM_FLEX, false>: (37, 24) with a (37, 1) column", "binary", [A((37, 24)), A((37, 1))], A((37, 24)), B_ALL, W5, nt=True)
_e("fast-binary-flex-row-col", "BinaryBody<.., OM_FLEX, OM_FLEX, false>: a (24,) row with a (37, 1) column", "binary", [A((24,)), A((37, 1))], A((37, 24)), B_ALL, W5,
   nt=True)
_e("fast-binary-bias", "BinaryBody<.., OM_VEC, OM_VEC, NT>, 2-D: (37, 24) + (24,), the row broadcast of a bias add (os = 0, is = 1)", "binary",
   [A((37, 24)), A((24,))], A((37, 24)), B_ALL, W5, nt=True)
for fdt in (f32, f64):
    for mname, mshape in (("dense", (37, 24)), ("row", (24,))):
        _e(f"fast-mask-left-{mname}-{fdt.name}", f"BinaryBody<BMul, {fdt.name}, .., b8, T, OM_VEC, OM_VEC, NT>: a {mname} bool mask times a float payload", "binary",
           [A(mshape, dt=b8), A((37, 24))], A((37, 24)), ("multiply",), (fdt,), nt=True)
        _e(f"fast-mask-right-{mname}-{fdt.name}", f"BinaryBody<BMul, {fdt.name}, .., T, b8, OM_VEC, OM_VEC, NT>: a float payload times a {mname} bool mask", "binary",
           [A((37, 24)), A(mshape, dt=b8)], A((37, 24)), ("multiply",), (fdt,), nt=True)
_e("fast-where-vec-scal", "k_ew_fast<WhereBody<T, b8, OM_VEC, OM_VEC, OM_SCAL>, 2>: relu's form", "where", [A((N1,), dt=b8), A((N1,)), K()], A((N1,)), ("where",), W5)
_e("fast-where-scal-vec", "WhereBody<T, b8, OM_VEC, OM_SCAL, OM_VEC>", "where", [A((N1,), dt=b8), K(), A((N1,))], A((N1,)), ("where",), W5)
_e("fast-where-vec-vec", "WhereBody<T, b8, OM_VEC, OM_VEC, OM_VEC>", "where", [A((N1,), dt=b8), A((N1,)), A((N1,))], A((N1,)), ("where",), W5)
_e("fast-where-scal-scal", "WhereBody<T, b8, OM_VEC, OM_SCAL, OM_SCAL>: a host scalar and one device element", "where", [A((N1,), dt=b8), K(), A((1,))], A((N1,)),
   ("where",), W5)
_e("fast-where-flex-col-cond", "WhereBody<T, b8, OM_FLEX, OM_FLEX, OM_FLEX>, U = 1: a (37, 1) column of conditions", "where", [A((37, 1), dt=b8), A((37, 24)), A((24,))],
   A((37, 24)), ("where",), W5)
_e("fast-where-flex-true", "WhereBody<.., OM_FLEX ..>: the condition a host scalar, true", "where", [K(True, dt=b8), A((N1,)), K()], A((N1,)), ("where",), W5)
_e("fast-where-flex-false", "WhereBody<.., OM_FLEX ..>: the condition a host scalar, false", "where", [K(False, dt=b8), K(), A((N1,))], A((N1,)), ("where",), W5)
CAST_PAIRS = [(s, d) for s in W5 for d in W5 if s != d]
_e("fast-cast-1d", "MD_CAST_FROM: k_ew_fast<UnaryBody<UCopy, D, D, S, OM_VEC, false>, 2>, 1203 elements (a tail of 3)", "cast", [A((N1,))], A((N1,)), ("astype",),
   CAST_PAIRS, nt=True)
_e("fast-cast-2d", "MD_CAST_FROM, 2-D: (37, 24) out of a row pitch of 32", "cast", [A((37, 32), cut=lambda a: a[:, :24])], A((37, 24)), ("astype",), CAST_PAIRS)
_e("fast-cast-mb3", "MD_CAST_FROM under max_blocks = 3: 2305 vectors + a tail of 1 (main loop, then the one-vector loop)", "cast", [A((9221,))], A((9221,)), ("astype",),
   CAST_PAIRS, max_blocks=3, trip=768)

# ---- k_ew_axes -------------------------------------------------------------------------------------------------------------------
S3, S4 = (5, 37, 356), (3, 5, 37, 120)
sliced3 = lambda dt=None: A((5, 40, 360), cut=lambda a: a[:, :37, :356], dt=dt)        # noqa: E731   (strides (14400, 360, 1): no two axes merge)
_ubw("axes-B1C", "k_ew_axes<AxBinary, 2>: (5, 37, 356) with (5, 1, 356); where: a mask vector, (5, 1, 356), (1, 37, 1)",
     lambda kind: [A(S3), A((5, 1, 356))] if kind == "binary" else [A(S3, dt=b8), A((5, 1, 356)), A((1, 37, 1))], A(S3), kinds="bw")
_ubw("axes-1R1", "k_ew_axes<AxBinary, 2>: (5, 37, 356) with (1, 37, 1), inner stride 0", lambda kind: [A((1, 37, 1)), A(S3)], A(S3), kinds="b")
_ubw("axes-4d", "k_ew_axes, four axes (e0 = 3): (3, 5, 37, 120) with (1, 5, 1, 120)",
     lambda kind: [A(S4), A((1, 5, 1, 120))] if kind == "binary" else [A(S4, dt=b8), A((1, 5, 1, 120)), K()], A(S4), kinds="bw")
_ubw("axes-sliced", "k_ew_axes<AxUnary, 1> / <AxBinary, 2> / <AxWhere, 3>: a sliced 3-D view, strides (14400, 360, 1)", _same(sliced3), A(S3))
_ubw("axes-scalar", "k_ew_axes with a host scalar operand (p == nullptr)",
     lambda kind: [sliced3(), K()] if kind == "binary" else [sliced3(b8), K(), sliced3()], A(S3), kinds="bw")
_ubw("axes-refuse-total", "generic kernels: (5, 37, 352) = 65120 elements, below 2^16",
     _same(lambda dt: A((5, 40, 356), cut=lambda a: a[:, :37, :352], dt=dt)), A((5, 37, 352)))
_ubw("axes-refuse-inner", "generic kernels: inner 358, % 4 != 0", _same(lambda dt: A((5, 40, 360), cut=lambda a: a[:, :37, :358], dt=dt)), A((5, 37, 358)))
_ubw("axes-refuse-stride", "generic kernels: an operand's outer stride 358, % 4 != 0", _same(lambda dt: A((5, 40, 358), cut=lambda a: a[:, :37, :356], dt=dt)), A(S3))
_ubw("axes-refuse-off", "generic kernels: an operand off alignment", _same(lambda dt: A((5, 40, 360), off=PAD + 1, cut=lambda a: a[:, :37, :356], dt=dt)), A(S3))
_e("axes-refuse-dtype", "k_binary_generic<.., double, ..>: an operand of another dtype (float32 with float64)", "binary", [sliced3(f32), sliced3()], A(S3), ("add", "less"), (f64,))

# ---- k_unary_tr ------------------------------------------------------------------------------------------------------------------
U_TR = ("copy", "negative", "absolute", "logical_not")
for R_, Cn in ((130, 127), (32, 512), (512, 32), (65, 257)):
    _e(f"tr-{R_}x{Cn}", f"k_unary_tr: out ({R_}, {Cn}) from a transposed source, {-(-R_ // 64)} x {-(-Cn // 64)} tiles", "unary", [A((Cn, R_), cut=lambda a: a.T)], A((R_, Cn)),
       U_TR, W5)
_e("tr-batched", "k_unary_tr, batched: out (3, 65, 95) from a (3, 95, 65) source with its last axes swapped", "unary", [A((3, 95, 65), cut=lambda a: a.transpose(0, 2, 1))],
   A((3, 65, 95)), U_TR, W5)
_e("tr-col-stride", "k_unary_tr: the source's column stride 135 > R = 130 (transpose of a sliced base)", "unary", [A((127, 135), cut=lambda a: a[:, :130].T)], A((130, 127)),
   U_TR, W5)
_e("tr-cast", "k_unary_tr<UCopy, double, double> reading int32: a converting transposed copy", "cast", [A((127, 130), cut=lambda a: a.T)], A((130, 127)), ("astype",),
   [(i32, f64), (f64, f32), (b8, i64)])
_e("tr-refuse-total", "k_unary_generic: (129, 127) = 16383 elements", "unary", [A((127, 129), cut=lambda a: a.T)], A((129, 127)), U_TR, W5)
_e("tr-refuse-R", "k_unary_generic: R = 31", "unary", [A((600, 31), cut=lambda a: a.T)], A((31, 600)), U_TR, W5)
_e("tr-refuse-Cn", "k_unary_generic: Cn = 31", "unary", [A((31, 600), cut=lambda a: a.T)], A((600, 31)), U_TR, W5)

# ---- the wide generic kernels ----------------------------------------------------------------------------------------------------
_ubw("generic-negative-strides", "k_*_generic: flipped operands (a[::-1])", _same(lambda dt: A((1203,), cut=lambda a: a[::-1], dt=dt)), A((1203,)))
_ubw("generic-permuted-4d", "k_*_generic: a permuted 4-D view", _same(lambda dt: A((6, 4, 7, 5), cut=lambda a: a.transpose(1, 3, 0, 2), dt=dt)), A((4, 5, 6, 7)))
_ubw("generic-step-2", "k_*_generic: step-2 slices on both axes", _same(lambda dt: A((74, 48), cut=lambda a: a[::2, ::2], dt=dt)), A((37, 24)))
_ubw("generic-8-axes", "k_*_generic: an 8-axis space that does not collapse ((2,) * 8 out of (3,) * 8)",
     _same(lambda dt: A((3,) * 8, cut=lambda a: a[:2, :2, :2, :2, :2, :2, :2, :2], dt=dt)), A((2,) * 8))
_ubw("generic-second-trip", "k_*_generic: 2048 * 256 + 300 elements with inner stride 2, a second grid trip",
     _same(lambda dt: A((2 * (GRID_TRIP + 300),), cut=lambda a: a[::2], dt=dt)), A((GRID_TRIP + 300,)), dtypes=(f32, b8), trip=GRID_TRIP // 4)
for cdt_, adt, bdt, op in ((f64, i32, f64, "add"), (f32, b8, f32, "add"), (i64, i32, i64, "add"), (i32, b8, i32, "add"), (b8, f32, i32, "logical_and"),
                           (f64, i32, i64, "true_divide")):
    _e(f"generic-mixed-{cdt_.name}-{op}", f"k_binary_generic<.., {cdt_.name} loop>: {adt.name} with {bdt.name}", "binary", [A((N1,), dt=adt), A((N1,), dt=bdt)], A((N1,)), (op,), (cdt_,))
_e("generic-mixed-unary", "k_unary_generic: logical_not of a dtype that is not the loop's storage type (bool)", "unary", [A((N1,))], A((N1,)), ("logical_not",),
   (f32, f64, i32, i64))
for cdt_ in (i32, f32, i64, f64):
    _e(f"generic-where-cond-{cdt_.name}", f"k_where_generic: a {cdt_.name} condition (NaN is true, -0.0 false)", "where", [A((N1,), dt=cdt_), A((N1,)), A((N1,))], A((N1,)),
       ("where",), W5)
_e("generic-fill-strided", "mdhip_fill into a strided view: k_unary_generic with a scalar source", "fill", [K()], A((74, 48), cut=lambda a: a[::2, ::2]), ("fill",), W5)
_e("generic-fill-step-2", "mdhip_fill into a[::2]", "fill", [K()], A((2406,), cut=lambda a: a[::2]), ("fill",), W5)

# ---- k_arange --------------------------------------------------------------------------------------------------------------------
AR4 = (i32, i64, f32, f64)
_e("arange-small", "k_arange: 1203 values", "arange", [], A((N1,)), ("arange",), AR4)
_e("arange-strided", "k_arange into a strided output view (a[::3])", "arange", [], A((3 * N1,), cut=lambda a: a[::3]), ("arange",), AR4)
_e("arange-second-trip", "k_arange: 2048 * 256 + 300 values, a second grid trip", "arange", [], A((GRID_TRIP + 300,)), ("arange",), AR4)

# ---- k_nw_unary / k_nw_binary ----------------------------------------------------------------------------------------------------
NW_U = ("negative", "absolute", "sign", "invert", "floor", "ceil", "sqrt", "isnan")
NW_B = B_ALL
for tag, length in (("lt-E", lambda E: E - 1), ("E", lambda E: E), ("E+1", lambda E: E + 1), ("2E-1", lambda E: 2 * E - 1), ("75E", lambda E: 75 * E),
                    ("75E+1", lambda E: 75 * E + 1), ("76E-1", lambda E: 76 * E - 1)):
    shape = lambda E, length=length: (length(E),)       # noqa: E731
    full = tag in ("lt-E", "75E+1", "76E-1")
    _e(f"nw-unary-{tag}", f"k_nw_unary<.., NT>: n = {tag} (E = 16 / element size)", "unary", [A(shape)], A(shape), NW_U if full else ("negative", "isnan"), N7, nt=True)
    _e(f"nw-vec-vec-{tag}", f"k_nw_binary<.., NM_VEC, NM_VEC, NT>: n = {tag}", "binary", [A(shape), A(shape)], A(shape), NW_B if full else B_GEOM, N7, nt=True)
    _e(f"nw-vec-scal-{tag}", f"k_nw_binary<.., NM_VEC, NM_SCAL, NT>: n = {tag}", "binary", [A(shape), K()], A(shape), NW_B if full else B_GEOM, N7, nt=True)
    _e(f"nw-scal-vec-{tag}", f"k_nw_binary<.., NM_SCAL, NM_VEC, NT>: n = {tag}", "binary", [K(), A(shape)], A(shape), NW_B if full else B_GEOM, N7, nt=True)
for nv in (NW_TRIP_VV + 1, 2 * NW_TRIP_VV + 5, 3 * NW_TRIP_VV + 1):
    shape = lambda E, nv=nv: (nv * E + E - 1,)          # noqa: E731
    _e(f"nw-vec-vec-nv{nv}", f"k_nw_binary<.., NM_VEC, NM_VEC, NT>: {nv} vectors + a tail of E - 1 past the cap of 1024 blocks (stride 262144): the two-in-flight loop", "binary",
       [A(shape), A(shape)], A(shape), B_GEOM, BY_SIZE, nt=True, trip=NW_TRIP_VV)
for nv in (NW_TRIP + 1, 2 * NW_TRIP + 5):
    shape = lambda E, nv=nv: (nv * E + 1,)              # noqa: E731
    _e(f"nw-unary-nv{nv}", f"k_nw_unary<.., NT>: {nv} vectors + a tail of 1 past the cap of 2048 blocks (stride 524288)", "unary", [A(shape)], A(shape), ("negative",), BY_SIZE,
       nt=True, trip=NW_TRIP)
    _e(f"nw-vec-scal-nv{nv}", f"k_nw_binary<.., NM_VEC, NM_SCAL, NT>: {nv} vectors + a tail of 1", "binary", [A(shape), K()], A(shape), B_GEOM, BY_SIZE, nt=True, trip=NW_TRIP)
    _e(f"nw-scal-vec-nv{nv}", f"k_nw_binary<.., NM_SCAL, NM_VEC, NT>: {nv} vectors + a tail of 1", "binary", [K(), A(shape)], A(shape), B_GEOM, BY_SIZE, nt=True, trip=NW_TRIP)
nw_n = lambda E: (75 * E + 1,)                           # noqa: E731
_ubw("nw-refuse-off", "k_nw_*_generic: an operand from element 1", _same(lambda dt: A(nw_n, off=PAD + 1, dt=dt)), A(nw_n), dtypes=N7, kinds="ub", uops=("negative", "isnan"))
_ubw("nw-refuse-out-off", "k_nw_*_generic: the output from element 1", _same(lambda dt: A(nw_n, dt=dt)), A(nw_n, off=PAD + 1), dtypes=N7, kinds="ub", uops=("negative", "isnan"))
_ubw("nw-refuse-strided", "k_nw_*_generic: a non-dense view (a[::2])", _same(lambda dt: A(lambda E: (150 * E + 2,), cut=lambda a: a[::2], dt=dt)), A(nw_n), dtypes=N7, kinds="ub",
     uops=("negative", "isnan"), bops=("add", "less", "multiply"))
_e("nw-refuse-mixed-storage", "k_nw_binary_generic: int8 with int16", "binary", [A((N1,), dt=i8), A((N1,), dt=i16)], A((N1,)), ("add", "less", "floor_divide"), (i16,))
_e("nw-u64-vs-negative-i64", "k_nw_binary_generic<.., __int128>: uint64 compared with int64 (negative values among them)", "binary", [A((N1,), dt=u64), A((N1,), dt=i64)],
   A((N1,)), CMP, (u64,))
_e("nw-i64-vs-u64", "k_nw_binary_generic<.., __int128>: int64 compared with uint64", "binary", [A((N1,), dt=i64), A((N1,), dt=u64)], A((N1,)), CMP, (u64,))
_e("nw-logical-not", "k_nw_unary_generic<ULogicalNot, uint8_t>: the carrier is not the storage type's", "unary", [A(nw_n)], A(nw_n), ("logical_not",), N7)

# ---- k_nw_binary_axes ------------------------------------------------------------------------------------------------------------
for tag, what, ins, oshape in (
        ("RC-C", "(37, 480) + (480,)", lambda: [A((37, 480)), A((480,))], (37, 480)),
        ("RC-R1", "(37, 480) + (37, 1)", lambda: [A((37, 480)), A((37, 1))], (37, 480)),
        ("BRC-B1C", "(3, 13, 480) x (3, 1, 480)", lambda: [A((3, 1, 480)), A((3, 13, 480))], (3, 13, 480)),
        ("4d", "(3, 5, 7, 160) x (1, 5, 1, 160)", lambda: [A((3, 5, 7, 160)), A((1, 5, 1, 160))], (3, 5, 7, 160)),
        ("scalar", "a (37, 480) view of a pitch of 496 with a host scalar", lambda: [A((37, 496), cut=lambda a: a[:, :480]), K()], (37, 480))):
    _e(f"nw-axes-{tag}", f"k_nw_binary_axes: {what}", "binary", ins(), A(oshape), ("add", "less", "floor_divide", "multiply"), N7)
_e("nw-axes-refuse-total", "k_nw_binary_generic: (34, 480) = 16320 elements", "binary", [A((34, 480)), A((480,))], A((34, 480)), B_GEOM, BY_SIZE)
_e("nw-axes-refuse-inner", "k_nw_binary_generic: inner 481, % E != 0 for every E", "binary", [A((37, 481)), A((481,))], A((37, 481)), B_GEOM, BY_SIZE)
_e("nw-axes-refuse-stride", "k_nw_binary_generic: an operand's row stride 481", "binary", [A((37, 481), cut=lambda a: a[:, :480]), A((480,))], A((37, 480)), B_GEOM, BY_SIZE)
_e("nw-axes-refuse-out-off", "k_nw_binary_generic: the output from element 1", "binary", [A((37, 480)), A((480,))], A((37, 480), off=PAD + 1), B_GEOM, BY_SIZE)

# ---- the narrow generic kernels --------------------------------------------------------------------------------------------------
_e("nw-generic-unary-2d", "k_nw_unary_generic: a 2-D view (there is no axes kernel for unary calls)", "unary", [A((37, 496), cut=lambda a: a[:, :480])], A((37, 480)), NW_U, N7)
for cdt_, bdt in ((i8, f16), (u16, i16), (f16, u64), (b8, u8)):
    _e(f"nw-where-{cdt_.name}-cond-{bdt.name}", f"k_nw_where_generic: a {cdt_.name} condition, {bdt.name} branches", "where", [A((N1,), dt=cdt_), A((N1,)), A((N1,))], A((N1,)),
       ("where",), (bdt,))
_e("nw-where-f16-scalars", "k_nw_where_generic<float>: scalar branches 0.1 / -2.3 rounded to float16 before they meet the loop", "where",
   [A((N1,), dt=b8), K(0.1), A((N1,))], A((N1,)), ("where",), (f16,))
_e("nw-where-f16-scalars-2", "k_nw_where_generic<float>: both branches scalars in a float16 output is not expressible (NumPy answers float64): array + -2.3", "where",
   [A((N1,), dt=i8), A((N1,)), K(-2.3)], A((N1,)), ("where",), (f16,))
for odt_, adt, bdt, op in ((b8, i8, u16, "less"), (i8, b8, i8, "add"), (u8, b8, u8, "add"), (i16, i8, u8, "add"), (u16, u8, u16, "add"), (i32, i16, u16, "add"),
                           (u32, u16, u32, "add"), (i64, i32, u32, "add"), (u64, u32, u64, "add"), (f16, i8, f16, "add"), (f32, i16, f16, "add"), (f64, i32, f16, "add")):
    _e(f"nw-generic-mixed-to-{odt_.name}", f"k_nw_binary_generic: {op}({adt.name}, {bdt.name}) -> {odt_.name}", "binary", [A((N1,), dt=adt), A((N1,), dt=bdt)], A((N1,)), (op,), (odt_,))

# ---- k_convert -------------------------------------------------------------------------------------------------------------------
for s in ALL12:
    carrier = "double" if s.kind == "f" else "uint64_t" if s.kind == "u" else "int64_t"
    _e(f"convert-from-{s.name}", f"k_convert<{carrier}>: {s.name} to each of the twelve dtypes, 1003 elements", "convert", [A((1003,))], A((1003,)), ("astype",),
       [(s, d) for d in ALL12])
for s, d, carrier in ((i16, f32, "int64_t"), (u32, i64, "uint64_t"), (f16, i32, "double"), (f64, f16, "double"), (f32, f16, "double")):
    _e(f"convert-strided-{s.name}-{d.name}", f"k_convert<{carrier}>: a strided 2-D view (a[::2, 1::3]) into a strided view", "convert",
       [A((60, 51), cut=lambda a: a[::2, 1::3])], A((30, 34), cut=lambda a: a[:, ::2]), ("astype",), [(s, d)])

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


def _twins(params):
    """Decorator: fn(case, mdopt, on_gpu) -> (CPU-double test, gpu-marked test), parametrised alike."""
    def deco(fn):
        @pytest.mark.parametrize("case", params)
        def cpu(lib, on_gpu, mdopt, case):
            if on_gpu:
                pytest.skip("other twin")
            fn(case, mdopt, False)

        @pytest.mark.gpu
        @pytest.mark.parametrize("case", params)
        def dev(lib, on_gpu, mdopt, case):
            assert on_gpu and lib.target == "hip:gfx950"
            fn(case, mdopt, True)
        return cpu, dev
    return deco


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    g, r = _bits(got), _bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]:#x}, expected {r[tuple(bad[0])]:#x}")


def _sentinel(dt):
    if dt.kind == "f":
        return dt.type(np.nan)
    if dt == b8:
        return np.True_
    return np.array([0x5A5A5A5A5A5A5A5A & ((1 << (8 * dt.itemsize - 1)) - 1)]).astype(dt)[0]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _counter(dt, n, salt):
    """Integers: an element counter times an odd constant, reinterpreted in the dtype (full range; neighbours always differ). bool:
    two bits of the same product."""
    with np.errstate(over="ignore"):
        c = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(7919 * salt)) * np.uint64(0x9E3779B97F4A7C15)
    if dt == b8:
        return (((c >> np.uint64(41)) ^ (c >> np.uint64(23))) & np.uint64(1)).astype(b8)
    if dt.itemsize == 8:
        return c.view(dt)
    odd = {1: 0x9D, 2: 0x9E37, 4: 0x9E3779B1}[dt.itemsize]
    with np.errstate(over="ignore"):
        c = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(7919 * salt)) * np.uint64(odd)
    return c.astype(np.dtype(f"u{dt.itemsize}")).view(dt)


def _spread(dt):
    return (-1, 1) if dt == f16 else (-3, 3)


def _floats(rng, dt, n):
    lo, hi = _spread(dt)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(dt)
    x[x == 0] = dt.type(1.25)
    return x


def _alphabet(dt):
    """A few values around the scalars of K: what an array holds where random numbers would leave the reference constant."""
    if dt.kind == "f":
        return np.array([1.5, -0.25, 3.0, -2.0, 0.0], dtype=dt)
    info = np.iinfo(dt)
    return np.array([3 if dt.kind == "u" else -3, 7, info.max, info.min, 0], dtype=dt)


def _positions(shape, V, trip):
    """Flat C-order indices where specials go: see the module docstring."""
    n = int(np.prod(shape, dtype=np.int64))
    if n == 0:
        return []
    nv = n // V
    P = {0, V - 1, nv * V - 1, nv * V, nv * V - V - 1, nv * V - V} | set(range(nv * V, n))
    for t in range(trip * V, n, trip * V):
        P |= {t - 1, t, t + V - 1}
    if len(shape) > 1:
        L = shape[-1]
        axes = []
        for d, e in enumerate(shape):
            if d == len(shape) - 1:
                idx = set(range(min(V, L))) | set(range(max(0, L - V), L)) | {63, 64}
            else:
                idx = {0, e // 2, e - 1} | ({63, 64} if d == len(shape) - 2 else set())
            axes.append(sorted(i for i in idx if 0 <= i < e))
        for tup in itertools.product(*axes):
            P.add(int(np.ravel_multi_index(tup, shape)))
    return sorted(p for p in P if 0 <= p < n)


def _specials(dt, op, k, full_shape, mixed, moving):
    """The special values operand k of `op` may hold (module docstring: Data, floats)."""
    sub = np.finfo(dt).smallest_subnormal
    nan, inf, z = np.nan, np.inf, 0.0
    if not full_shape:
        s = [nan, sub, -sub]
    elif op == "sqrt":
        s = [nan, inf, z, -z, sub]
    elif op in ("floor_divide", "mod"):
        s = [nan, z, -z, sub, -sub]
    elif mixed:
        s = [nan, z, -z, sub, -sub]
    else:
        s = [nan, inf, -inf, z, -z, sub, -sub]
    if op in ("floor_divide", "mod") and k == 1:
        s = []
    if op == "subtract" and k == 1:
        s = [v for v in s if v == v]
    out = np.array(s, dtype=dt)
    if moving and dt.itemsize >= 4 and len(out):         # a bit-moving call keeps a NaN's payload and sign
        payload = np.array([0xFFC12345 if dt == f32 else 0xFFF8000012345678], dtype=np.dtype(f"u{dt.itemsize}")).view(dt)
        out = np.concatenate([out, payload])
    return out


def _values(e, op, k, dt, shape, oshape, rng, mixed, n_float_full, V, draw=0):
    """Operand k of `op`, of dtype dt and (view) shape `shape`."""
    n = int(np.prod(shape, dtype=np.int64))
    with_scalar = any(isinstance(s, K) for s in e.ins) and op not in ("add", "subtract", "multiply", "true_divide", "where")
    if (op in ("equal", "not_equal") or with_scalar) and dt != b8:
        x = _alphabet(dt)[rng.integers(0, 5, n)]
        if op in ("floor_divide", "mod") and k == 1:
            x[x == 0] = 7
    elif dt.kind == "f":
        x = _floats(rng, dt, n)
    else:
        x = _counter(dt, n, k + 1 + 31 * draw).copy()
    cond_like = e.kind == "where" and k == 0
    if (op in LOGICAL or op == "logical_not" or cond_like) and dt != b8:
        x[rng.random(n) < 0.5] = 0
    if op == "sqrt":
        x = np.abs(x)
    if op == "sign" and dt.kind in "iu":
        x[rng.random(n) < 0.3] = 0
    if op == "isnan" and dt.kind == "f":
        x[rng.random(n) < 0.3] = np.nan
    if op in ("floor_divide", "mod", "true_divide") and k == 1 and dt.kind != "f":
        x[x == 0] = 3
    if dt.kind == "f" and n > 1:                         # (a one-element operand stays an ordinary number)
        full = tuple(shape) == tuple(oshape)
        sp = _specials(dt, op, k, full, mixed, moving=op in ("copy", "where") and not cond_like)
        if len(sp):
            P = _positions(shape, V, e.trip)
            if full and n_float_full > 1:                # operands of the output's shape share the positions between them
                P = P[(k + e.ops.index(op)) % n_float_full::n_float_full]
            if 2 * len(P) > n:                           # (a handful of elements: every other one stays an ordinary number)
                P = P[::2]
            for j, p in enumerate(P):
                x[p] = sp[(j + k) % len(sp)]
    return x.reshape(shape)


def _cast_values(src, dst, n, rng, V, trip, draw=0):
    """n values of dtype src, in range of dst, with the rounding cases of the module docstring."""
    if dst == b8:
        if src.kind == "f":
            x = _floats(rng, src, n)
            x[rng.random(n) < 0.5] = 0
            sp = np.array([0.5, -0.0, np.nan, np.finfo(src).smallest_subnormal, 0.0, -np.inf], dtype=src)
            for j, p in enumerate(_positions((n,), V, trip)):
                x[p] = sp[j % len(sp)]
            return x
        x = _counter(src, n, 3 + 31 * draw).copy()
        x[rng.random(n) < 0.5] = 0
        return x
    if src == b8:
        return _counter(b8, n, 3 + 31 * draw)
    if dst.kind in "iu":
        di = np.iinfo(dst)
        lo, hi = di.min, di.max
        if src.kind in "iu":
            si = np.iinfo(src)
            lo, hi = max(lo, si.min), min(hi, si.max)
            x = rng.integers(lo, hi, n, dtype=np.int64 if hi <= np.iinfo(np.int64).max else np.uint64, endpoint=True).astype(src)
            x[:2] = (lo, hi)
            return x
        exact = 1 << (np.finfo(src).nmant + 1)           # every integer up to here is a value of src
        lo, hi = max(lo, -exact), min(hi, exact)
        v = rng.integers(lo, hi, n, endpoint=True).astype(np.float64)
        small = np.abs(v) < exact / 8
        frac = rng.integers(0, 4, n) / 4.0               # truncation toward zero: the fraction goes away from zero, and not past lo
        v = np.where(small, v + np.sign(v) * frac, v)
        v[:2] = (lo, hi)
        if dst.kind == "u":
            v = np.abs(v)
        v = np.clip(v, lo, hi)
        x = v.astype(src)
        assert np.array_equal(x.astype(np.float64), v)
        return x
    # float destination
    if src.kind in "iu":
        x = _counter(src, n, 3 + 31 * draw).copy()
        if dst == f16:
            x = (x.astype(np.int64) % 120001 - 60000 if src.kind == "i" else x % 60001).astype(src) if src.itemsize > 1 else x
        edge = []
        for p in (24, 53, 11):
            edge += [(1 << p) - 1, 1 << p, (1 << p) + 1, (1 << p) + 2, (1 << p) + 3, 3 * (1 << p) + 1, 3 * (1 << p) + 3]
        info = np.iinfo(src)
        edge = [v for v in edge + [-v for v in edge] if info.min <= v <= info.max and (dst != f16 or abs(v) <= 60000)]
        x[:len(edge)] = np.array(edge[:n], dtype=src)[:len(x)]
        return x
    lo, hi = max(_spread(src)[0], _spread(dst)[0]), min(_spread(src)[1], _spread(dst)[1])
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(src)
    sp = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(src).smallest_subnormal]
    if np.finfo(src).nmant > np.finfo(dst).nmant:        # ties, just above / below a tie, overflow to inf, subnormal results
        u, tiny, big = 2.0 ** -np.finfo(dst).nmant, float(np.finfo(dst).smallest_subnormal), float(np.finfo(dst).max)
        sp += [1 + u / 2, 1 + 3 * u / 2, -(1 + u / 2), 1 + u / 2 + 2.0 ** -np.finfo(src).nmant, 1 + 3 * u / 2 - 2.0 ** -np.finfo(src).nmant,
               tiny * 2.5, tiny * 3.5, tiny * 0.5, tiny * 0.75, tiny * 1024.5, big * (1 + u / 4), big * (1 + u / 2), -big * (1 + u)]
    sp = np.array(sp, dtype=np.float64).astype(src)
    for j, p in enumerate(_positions((n,), V, trip) + list(range(20, 20 + 2 * len(sp)))):
        if p < n:
            x[p] = sp[j % len(sp)]
    return x


# ---- one call --------------------------------------------------------------------------------------------------------------------
class Call:
    """One (entry, dtype item, op): NumPy operands inside their bases, the reference, the expected output base."""

    def __init__(self, e, item, op):
        # (a small operand — a handful of bools — can be its own rolled copy by chance: the data is the first draw, in a fixed order of
        # seeds, that is position sensitive; the CPU twin asserts the condition for every size)
        for draw in range(64):
            self.build(e, item, op, draw)
            if sum(v.size for v in self.views.values()) > 4096 or not self.insensitive():
                break

    def build(self, e, item, op, draw):
        self.e, self.op = e, op
        pair = e.kind in ("cast", "convert")
        self.loop_dt = item[0] if pair else item
        self.E = max(1, 16 // self.loop_dt.itemsize) if self.loop_dt in N7 and not pair else 4
        E = self.E
        self.in_dts = [(s.dt or self.loop_dt) for s in e.ins]
        rng = np.random.default_rng([TABLE.index(e), self.loop_dt.num, e.ops.index(op), item[1].num if pair else 0, draw])
        self.oshape = np.empty(e.out.dense_shape(E), dtype=np.bool_)
        self.oshape = (self.oshape if e.out.cut is None else e.out.cut(self.oshape)).shape
        arrs = [k for k, s in enumerate(e.ins) if isinstance(s, A)]
        mixed = len({self.in_dts[k] for k in arrs}) > 1 and e.kind == "binary"
        vshape = {k: e.ins[k].view(np.empty(e.ins[k].base_len(E), dtype=np.bool_), E).shape for k in arrs}
        n_full = sum(1 for k in arrs if self.in_dts[k].kind == "f" and tuple(vshape[k]) == tuple(self.oshape))
        self.bases, self.views, self.scalars = {}, {}, {}
        for k, s in enumerate(e.ins):
            dt = self.in_dts[k]
            if isinstance(s, K):
                self.scalars[k] = s.get(dt, op, k)
                continue
            base = np.full(s.base_len(E), _sentinel(dt), dtype=dt)
            view = s.view(base, E)
            assert np.shares_memory(view, base) or view.size == 0
            if pair:
                vals = _cast_values(item[0], item[1], view.size, rng, 4, e.trip, draw).reshape(view.shape)
            else:
                vals = _values(e, op, k, dt, view.shape, self.oshape, rng, mixed, n_full, E, draw)
            view[...] = vals
            self.bases[k], self.views[k] = base, view
        if e.kind == "fill":
            self.odt = self.loop_dt
        elif e.kind == "arange":
            self.odt = self.loop_dt
            self.start, self.step = (-3.5, 0.25) if self.loop_dt.kind == "f" else (-7, 3)
        elif pair:
            self.odt = item[1]
        self.ref = self.reference(self.views)
        self.odt = self.ref.dtype
        self.obase = np.full(e.out.base_len(E), _sentinel(self.odt), dtype=self.odt)
        self.expect = self.obase.copy()
        e.out.view(self.expect, E)[...] = self.ref

    def np_operand(self, views, k):
        return views[k] if k in views else self.in_dts[k].type(self.scalars[k])

    def reference(self, views):
        e, op = self.e, self.op
        with np.errstate(all="ignore"):
            if e.kind == "unary":
                r = self.np_operand(views, 0).copy() if op == "copy" else _np_fn(op)(self.np_operand(views, 0))
            elif e.kind == "binary":
                r = _np_fn(op)(self.np_operand(views, 0), self.np_operand(views, 1))
            elif e.kind == "where":
                a, b = (views[k] if k in views else self.scalars[k] for k in (1, 2))     # (weak Python scalars, as the public call passes them)
                if 1 not in views and 2 not in views:
                    a = self.in_dts[1].type(a)
                r = np.where(self.np_operand(views, 0), a, b)
            elif e.kind in ("cast", "convert"):
                r = views[0].astype(self.odt)
            elif e.kind == "fill":
                r = np.full(self.oshape, self.scalars[0], dtype=self.odt)
            else:
                n = self.oshape[0]
                r = np.arange(self.start, self.start + n * self.step, self.step, dtype=self.odt)
                assert r.shape == (n,)
        return np.ascontiguousarray(np.broadcast_to(r, self.oshape))

    def insensitive(self):
        """The (operand, axis) pairs along which a roll by one leaves the reference as it is."""
        same = []
        for k, v in self.views.items():
            for ax in range(v.ndim):
                if v.shape[ax] > 1:
                    rolled = dict(self.views)
                    rolled[k] = np.roll(v, 1, axis=ax)
                    if np.array_equal(_bits(self.reference(rolled)), _bits(self.ref)):
                        same.append((k, ax))
        return same

    def check_sensitive(self):
        """Rolling any array operand by one along any axis longer than 1 changes the reference."""
        same = self.insensitive()
        assert not same, (self.e.id, self.loop_dt.name, self.op, f"(operand, axis) {same}: rolled by one, same reference")

    # -- device side --
    def upload(self):
        E = self.E
        self.dbases = {k: nd.asarray(b) for k, b in self.bases.items()}
        self.dviews = {k: self.e.ins[k].view(self.dbases[k], E) for k in self.bases}
        for k, v in self.dviews.items():
            assert v._buf is self.dbases[k]._buf and v.shape == self.views[k].shape, (self.e.id, k)

    def scalar_desc(self, k):
        v = self.scalars[k]
        return nd._scalar_desc(v, _capi.F64 if isinstance(v, float) else _capi.I64)

    def desc(self, k):
        return self.dviews[k].desc(self.oshape) if k in self.dviews else self.scalar_desc(k)

    def run_capi(self):
        """The call as ndarray.py makes it at its end, into a sentinel base of this module's own -> the whole base."""
        e, op, lib = self.e, self.op, nd._lib()
        dob = nd.asarray(self.obase)
        out = e.out.view(dob, self.E)
        assert out._buf is dob._buf and out.shape == self.oshape
        od = out.desc()
        if e.kind == "unary":
            narrow = self.in_dts[0] in N7 or self.odt in N7
            if op == "copy" and narrow:
                lib.convert(self.desc(0), od)
            else:
                lib.unary(U_CODE[op], self.desc(0), od)
        elif e.kind == "binary":
            loop = _np_fn(op).resolve_dtypes((self.in_dts[0], self.in_dts[1], None))
            assert loop[2] == self.odt
            lib.binary(B_CODE[op], self.desc(0), self.desc(1), od, nd.dtype_code(loop[0]))
        elif e.kind == "where":
            lib.where(self.desc(0), self.desc(1), self.desc(2), od)
        elif e.kind == "cast":
            lib.unary(_capi.U_COPY, self.desc(0), od)
        elif e.kind == "convert":
            lib.convert(self.desc(0), od)
        elif e.kind == "fill":
            lib.fill(od, self.scalar_desc(0))
        elif out.size:
            lib.arange(od, float(self.start), float(self.step))
        return dob.get()

    def run_public(self):
        """The same call through nd.* -> the result array (fill: the whole base)."""
        e, op = self.e, self.op
        arg = lambda k: self.dviews[k] if k in self.dviews else self.scalars[k]      # noqa: E731
        if e.kind == "unary":
            if 0 not in self.dviews:
                return nd.full(self.oshape, self.scalars[0], dtype=self.odt).get()
            x = arg(0) if self.dviews[0].shape == self.oshape else nd.broadcast_to(arg(0), self.oshape)
            return (nd.copy(x) if op == "copy" else getattr(nd, op)(x)).get()
        if e.kind == "binary":
            return getattr(nd, op)(arg(0), arg(1)).get()
        if e.kind == "where":
            a, b = arg(1), arg(2)
            if 1 not in self.dviews and 2 not in self.dviews:
                a = self.in_dts[1].type(a)
            return nd.where(arg(0), a, b).get()
        if e.kind in ("cast", "convert"):
            return self.dviews[0].astype(self.odt).get()
        if e.kind == "fill":
            dob = nd.asarray(self.obase)
            e.out.view(dob, self.E).fill(self.scalars[0])
            return dob.get()
        n = self.oshape[0]
        return nd.arange(self.start, self.start + n * self.step, self.step, dtype=self.odt).get()


def _items(e):
    for item in e.dtypes:
        for op in e.ops:
            if e.kind in ("unary", "binary") and len({(s.dt or item) for s in e.ins}) == 1 and not _valid(op, item):
                continue
            yield item, op


def _check_entry(case, mdopt, on_gpu, public=False):
    e = BY_ID[case]
    if on_gpu and e.max_blocks:
        mdopt("max_blocks", e.max_blocks)
    ran = 0
    for item, op in _items(e):
        c = Call(e, item, op)
        ran += 1
        what = (e.id, getattr(item, "name", None) or (item[0].name, item[1].name), op)
        if not on_gpu and not public:
            c.check_sensitive()
        c.upload()
        for nt in ((0, 1) if e.nt and on_gpu else (None,)):
            if nt is not None:
                mdopt("nt", nt)
            if public and e.kind != "fill":
                _same_bits(c.run_public(), c.ref, what + ("public", nt))
            elif public:
                _same_bits(c.run_public(), c.expect, what + ("public", nt))
            else:
                _same_bits(c.run_capi(), c.expect, what + (nt,))
        if nt is not None:
            mdopt("nt", -1)
    assert ran, e.id


BOTH = [e.id for e in TABLE if not e.gpu_only]
GPU_ONLY = [e.id for e in TABLE if e.gpu_only]

test_paths, test_paths_gpu = _twins(BOTH)(_check_entry)
test_public, test_public_gpu = _twins(BOTH)(lambda case, mdopt, on_gpu: _check_entry(case, mdopt, on_gpu, public=True))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_ONLY)
def test_default_grid_gpu(lib, on_gpu, mdopt, case):
    """The entries that need the product library's own grid (docstring: not run on both twins); the reference is NumPy's all the same."""
    assert on_gpu and lib.target == "hip:gfx950"
    _check_entry(case, mdopt, True)
    _check_entry(case, mdopt, True, public=True)


def test_table_is_complete():
    """Every kernel family and template form the issue names has an entry; every id is unique; every entry names what it reaches."""
    text = " ".join(e.reaches for e in TABLE)
    for name in ("k_ew_fast", "UnaryBody", "BinaryBody", "WhereBody", "OM_VEC", "OM_SCAL", "OM_FLEX", "MD_CAST_FROM", "k_ew_axes", "k_unary_tr", "k_unary_generic",
                 "k_binary_generic", "k_where_generic", "k_arange", "k_convert<int64_t>", "k_convert<uint64_t>", "k_convert<double>", "k_nw_unary<", "k_nw_binary<",
                 "k_nw_binary_axes", "k_nw_unary_generic", "k_nw_binary_generic", "k_nw_where_generic", "__int128"):
        assert name in text, name
    assert all(e.reaches and e.dtypes and e.ops for e in TABLE)
