"""Every launch form of the float16 / int8 / uint8 matmul (csrc/gemm_narrow.hip and the narrow half of csrc/gemm.hip: md_narrow_layout,
plan_narrow, plan_narrow_declined, plan_widened, run_step's S_NMFMA / S_NGENERIC / S_NCONV) against exact references — the companion of
tests/test_matmul_paths.py, whose method it keeps; the thin and long-k hand-offs of these types (skinny.hip) are tests/test_narrow_thin.py's.

The centre is TABLE: what an entry reaches (kernel names with their template arguments, as a kernel trace prints them, or the route:
`matmul(narrow, conversion) x2 + <wide kernel> + matmul(narrow, conversion)`), the kind (f16, f16->f32, i8, i8->i32, u8: operand type -> type of
C), M, K, N, batch, the layout of A and B ("NN" .. "TT": which of them is stored transposed), how A, B and C sit in their base arrays (Op,
C_LAYOUTS) and the options set through the `mdopt` fixture. There is no hook that reports which kernel ran: `reaches` is derived per entry
by _route, a restatement of md_build_gemm's batch fold, md_narrow_layout, plan_narrow's hand-off floors (md_gemm_longk, md_gemm_skinny) and
plan_narrow_declined; the wide kernel of the widened route comes from test_matmul_paths' restatement of plan_mfma with the 64 x 64 tile
forced (gemm_cfg = 1). The table is built for bases that start on a 16-B boundary; on the device every call restates the route from the real
byte addresses of its views (desc().data) and must find the table's `reaches` again, so nothing is assumed about how the allocator aligns a
base. It is to be confirmed by a kernel trace of the gpu half (profiles/README.md: narrow_matmul_paths_kernel_stats.csv).
The calls go through the C-ABI (lib.matmul on descriptors): that is what takes a strided C. test_public_functions runs a subset through
nd.matmul, with and without `out=` / `dtype=`.

The constants the shapes come from (gemm_narrow.hip): block tile 128 x 128; k-tile BK = 128 B of every operand row = 64 (float16) / 128
(int8, uint8) of k; a 16-B chunk = epc = 8 / 16 elements, the unit of the DMA and of every EDGE predicate; the k loop is unrolled by two
(prologue, odd-tail and even-tail exits: k-tile counts 1 .. 5 reach each and a second trip); blocks map to tiles through (xcd, q, r) of the
tile count (tile counts 1, 2, 3, 7, 8, 9, 10, 15, 17: r = 0 and r != 0, q = 0 and q > 0; these `map-` entries alone are longer than three
tiles on a side). plan_narrow_declined: thin = min(M, N) <= 8; few_long = float16 and K / 1024 (8.8 - tiles / 2) > 22.5; small = K <= 512 and
batch M N K <= 2^22; md_longk_shape. Not reached: md_narrow_layout's `step * esz * 8 < 2^31` limit — a row step of 256 MiB needs gigabytes
of base.

What every entry checks:
  exact data     int8 / uint8: full-range random bytes with the extremes planted; the expected result is the exact integer product (a
                 float64 product of values below 2^53) cast to the output type: the low byte, or NumPy's int32 wrap; array_equal.
                 float16: operands from the ODD values {-3, -1, 1, 3} ({-1, 1} where K is in the thousands): every partial sum in any
                 order is an exact integer in float32, the expected result is the float64 product cast once to the output type, compared
                 bit for bit. For float16 outputs the module asserts |exact| <= 2048 on its own data — a precondition of the data, not a
                 tolerance: then the cast is exact too, and one dropped or doubled term flips an output's parity.
  surroundings   A, B and C are views of larger bases. Padding of A and B is NaN (float16) or random bytes: a lane that reads past its
                 operand and lets it reach C fails the exact check. Every byte of C's base, view included, is 0xA5 before the call:
                 afterwards the view equals the reference and every byte outside it is still 0xA5 — with the exact result that is also
                 what shows every tile of the block-to-tile map written exactly once.
  the pool       before a call that takes the widened route, blocks of exactly its temporaries' byte sizes (ba M K, bb K N, batch M N
                 times the wide size, the wide plan's split-k / long-k partials) are allocated, filled with NaN and freed.
  float data     float16 kinds, standard normals, against the float64 product under the project's contract (tests/test_narrow_thin.py
                 _check): |got - exact| <= ulp16(exact) / 2 + K 2^-23 (|a| @ |b|) (float32 output: ulp32), finite where the reference
                 is. The largest error / bound per `reaches` goes to the file MDHIP_NARROW_PATHS_REPORT names
                 (profiles/narrow_matmul_paths_error.txt holds the device run's).
  generic f16    k_gemm_narrow_generic<_Float16, float> / k_gemm_widen_generic<_Float16, float> claim an fma chain in k order in float32:
                 on the float data they equal, bit for bit, a float32 accumulator updated for k = 0 .. K-1 with the float32 product of the
                 two float16 values (exact in float32, so fma and multiply-add agree), cast once.
Bit identity (float data, f16 and f16->f32, 2 and 3 k-tiles): the four layouts of one product give the same bits (gemm_narrow.hip: the KC
read and the transposed reads hand the same k to element j of a lane), and so does a whole-tile product run as itself and as the top-left
tiles of an EDGE problem one chunk larger in M and N. The widened entries that split k, and three MFMA entries, run three times interleaved
with each other and must repeat their bits.
Mutation check (scratch builds of gemm_narrow.hip, not kept; the gpu half of this module against each):
  (1) the k loop one k-tile short (nk - 1): all 516 entries on k_gemm_narrow_mfma / k_gemm_widen_mfma fail, with the 24 public and the 4
      bit-identity cases that run them; no generic, widened or long-k entry does.
  (2) `kr <= K` for `kr < K` in stage<>'s EDGE predicate of the MN image: 71 entries fail, every one EDGE with a ragged last k-tile and an MN
      operand — all such TN entries (both operands read the k-row behind their last) and the float16 ones of NN / TT (NaN filler times the
      other operand's zero chunk). The 41 int8 / uint8 NN / TT entries of that form pass, and rightly: the stray k-row meets the zero chunk
      of the KC operand, and an integer 0 x anything is 0 — there the mutant still computes the product. (The bases end in a stored row of
      filler so that such a read stays inside them.)
  (3) `n + 16 <= g.N + 1` in the int8 write-out: the five c_vec entries with N % 16 = 15 (143, 255, 271) fail by the sentinel behind their
      rows, nothing else — N = 130 alone does not see this one.
  (4) q and q + 1 swapped in the tile map: run on the 277 EDGE entries only, whose loads and stores are guarded (the swapped map names tiles
      past the grid, which a whole-tile launch would write out of bounds): all 204 of more than one tile fail, r = 0 included, the 73
      single-tile ones pass.

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound; entries with batch M N K <= 2^24 only: the double is a triple
loop) — it proves data and references right — and gpu-marked on the product library.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import test_matmul_paths as wide_paths      # the restatement of the wide plan (plan_mfma, in-kernel split-K) the widened route lands on
from minidiff_amd import ndarray as nd

f16, f32, i8, u8, i32 = (np.dtype(t) for t in (np.float16, np.float32, np.int8, np.uint8, np.int32))
# kind -> (operand dtype, dtype of C)
KINDS = {"f16": (f16, f16), "f16->f32": (f16, f32), "i8": (i8, i8), "i8->i32": (i8, i32), "u8": (u8, u8)}
CPU_MAX = 1 << 24
TILE = 128
LAYS = ("NN", "NT", "TN", "TT")
_twins = wide_paths._twins


def _b(x):
    return "true" if x else "false"


def _up(n, m):
    return -(-n // m) * m


class Op:
    """How an operand sits in its base: `pad` extra elements per stored row (the row length is first rounded up to a 16-B chunk), `off`
    elements in front of it, `bpad` extra elements per batch; kind: None | "step2" (every other stored column: both strides non-unit) |
    "flip" (negative stride along the stored columns) | "bcast" (stride 0 across the stored rows); `one`: a single batch, broadcast over
    the batch of C (a_bs / b_bs = 0)."""
    def __init__(self, pad=0, off=0, bpad=0, kind=None, one=False):
        self.pad, self.off, self.bpad, self.kind, self.one = pad, off, bpad, kind, one


PLAIN = Op()
# C layouts -> (offset, c_bs, c_ms, c_ns) in elements; e = elements of C per 16 B
C_LAYOUTS = {
    "contig": lambda M, N, e: (0, M * N, N, 1),
    "ms+16B": lambda M, N, e: (0, M * (_up(N, e) + e), _up(N, e) + e, 1),       # rows stay on 16 B: c_vec holds
    "ms+1": lambda M, N, e: (0, M * (N + 1), N + 1, 1),
    "off1": lambda M, N, e: (1, M * N, N, 1),
    "T": lambda M, N, e: (0, N * (M + e), 1, M + e),
    "bpad": lambda M, N, e: (0, _up(M * N, e) + e, N, 1),                       # a padded batch step, still on 16 B
}
C_ALL = tuple(C_LAYOUTS)


def _geometry(rows, cols, nbatch, op, epc):
    """An operand stored as nbatch x rows x cols -> (elements of the base, offset, batch / row / column strides)."""
    cs = 2 if op.kind == "step2" else -1 if op.kind == "flip" else 1
    ld = _up(cols * abs(cs), epc) + op.pad
    rs = 0 if op.kind == "bcast" else ld
    bs = (1 if op.kind == "bcast" else rows) * ld + op.bpad
    off = op.off + (cols - 1 if cs < 0 and cols else 0)
    # (a stored row and a chunk of filler behind the last batch: a lane that reads one row past its operand reads filler)
    return op.off + nbatch * bs + ld + epc, off, (bs, rs, cs)


# ---- the restatement: md_build_gemm's fold, plan_narrow, plan_narrow_declined, plan_widened ------------------------------------------------
CT_NAME = {"f16": "(anonymous namespace)::MdThin<_Float16, _Float16>", "f16->f32": "(anonymous namespace)::MdThin<_Float16, float>",
           "i8": "(anonymous namespace)::MdThin<signed char, signed char>", "i8->i32": "(anonymous namespace)::MdThin<signed char, int>",
           "u8": "(anonymous namespace)::MdThin<signed char, signed char>"}
GENERIC_T = {f16: "_Float16, float", i8: "signed char, int", u8: "unsigned char, int"}
CONV = "matmul(narrow, conversion)"


def _gemm(e, pa=0, pb=0, pc=0):
    """md_build_gemm on the entry's views (pa / pb / pc: byte addresses of the three bases): element strides, a_bs / b_bs = 0 for a single
    batch, and B broadcast over a batch laid out as more rows of A and C folded into ONE product of batch M rows."""
    dt, ct = KINDS[e.kind]
    epc, ce = 16 // dt.itemsize, 16 // ct.itemsize
    _, a_off, (a_bs, a_r, a_c) = _geometry(*((e.K, e.M) if e.lay[0] == "T" else (e.M, e.K)), 1 if e.a.one else e.batch, e.a, epc)
    _, b_off, (b_bs, b_r, b_c) = _geometry(*((e.N, e.K) if e.lay[1] == "T" else (e.K, e.N)), 1 if e.b.one else e.batch, e.b, epc)
    c_off, c_bs, c_ms, c_ns = C_LAYOUTS[e.c](e.M, e.N, ce)
    g = SimpleNamespace(batch=e.batch, M=e.M, N=e.N, K=e.K, a=pa + a_off * dt.itemsize, b=pb + b_off * dt.itemsize, c=pc + c_off * ct.itemsize,
                        a_bs=0 if (e.a.one or e.batch == 1) else a_bs, b_bs=0 if (e.b.one or e.batch == 1) else b_bs, c_bs=c_bs, c_ms=c_ms, c_ns=c_ns)
    g.a_ms, g.a_ks = (a_c, a_r) if e.lay[0] == "T" else (a_r, a_c)
    g.b_ks, g.b_ns = (b_c, b_r) if e.lay[1] == "T" else (b_r, b_c)
    g.ba, g.bb = (1 if g.a_bs == 0 else e.batch), (1 if g.b_bs == 0 else e.batch)       # (plan_widened's batches of its temporaries)
    if g.batch > 1 and g.b_bs == 0 and g.M > 0 and g.a_bs == g.M * g.a_ms and g.c_bs == g.M * g.c_ms:
        g.M, g.batch, g.a_bs, g.c_bs, g.ba = g.M * g.batch, 1, 0, 0, 1
    return g


def _narrow_layout(g, esz):
    """md_narrow_layout -> (ok, a_kc, b_kc, edge), without the 2^31 lane-offset limit"""
    epc = 16 // esz

    def side(p, rows, rs, ks, bs):
        if p % 16 or (bs * esz) % 16:
            return None
        if ks == 1 and g.K % epc == 0:
            kc, step = True, rs
        elif rs == 1 and rows % epc == 0:
            kc, step = False, ks
        else:
            return None
        return kc if step > 0 and (step * esz) % 16 == 0 else None
    a_kc, b_kc = side(g.a, g.M, g.a_ms, g.a_ks, g.a_bs), side(g.b, g.N, g.b_ns, g.b_ks, g.b_bs)
    return a_kc is not None and b_kc is not None, a_kc, b_kc, bool(g.M % TILE or g.N % TILE or g.K % (128 // esz))


def _longk_shape(M, K, N):
    big = max(M, N)
    return M <= 128 and N <= 128 and (K >= 512 if big <= 8 else (K >= 8192 and K >= 64 * big))


def _few_long(K, blocks):
    return (K / 1024.0) * (8.8 - 0.5 * float(blocks)) > 22.5


def _longk_kernels(T, M, K, N, batch, itemsize):
    """longk_dispatch / longk_run -> (kernel names, bytes of the block partials)"""
    big = max(M, N)
    tm, tn = ((1, 1) if (M, N) == (1, 1) else (2, 2) if big <= 2 else (4, 4) if big <= 4 else (8, 1) if N == 1 else (1, 8) if M == 1 else (8, 8))
    patches = batch * -(-M // tm) * -(-N // tn)
    nb = min(-(-K // 4096), 1 if patches >= 1024 else 1024 // patches)
    nb = -(-K // -(-K // nb))
    return f"k_longk_partial<{T}, {tm}, {tn}> + k_longk_finish<{T}, {tm}, {tn}>", patches * nb * tm * tn * itemsize


def _skinny_floors(g):
    """md_gemm_skinny's shape floors (what it takes above them is tests/test_narrow_thin.py's): True if the hand-off may take the product"""
    if g.N <= 8 < g.M:
        R = g.M
    elif g.M <= 8 < g.N:
        R = g.N
    else:
        return False
    return R >= 512 and g.K >= 64 and R * g.K * g.batch >= (1 << 20)


def _route(e, g):
    """plan_narrow on the descriptor g -> (reaches, bytes of the temporaries the plan takes)."""
    dt, ct = KINDS[e.kind]
    esz, wide_out = dt.itemsize, ct != dt
    o = {**DEFAULTS, **e.opts}
    native = not wide_out or o["gemm_widen"] != 0
    if o["gemm_narrow_skinny"] and g.K > 0 and native:                      # the hand-offs on the operands as they are
        small = min(g.M, g.N)
        if _longk_shape(g.M, g.K, g.N) and not (dt == f16 and max(g.M, g.N) > 8 and small >= 64):
            k, p = _longk_kernels(CT_NAME[e.kind], g.M, g.K, g.N, g.batch, 4)
            return k, [p]
        assert not _skinny_floors(g), (e.id, "above the thin hand-off's floors: not this module's")
    ok, a_kc, b_kc, edge = _narrow_layout(g, esz)
    blocks = -(-g.M // TILE) * -(-g.N // TILE) * g.batch
    thin, few_long = g.M <= 8 or g.N <= 8, esz == 2 and _few_long(g.K, blocks)
    if native and ok and g.K > 0 and not thin and not few_long and not (esz == 1 and _longk_shape(g.M, g.K, g.N)):
        name = f"k_gemm_{'widen' if wide_out else 'narrow'}_mfma<{esz}, {_b(a_kc)}, {_b(b_kc)}, {_b(edge)}>"
        if esz == 1 and not wide_out:       # launch_mfma's c_vec: the int8 write-out's 16-B row pieces, or its byte loop
            c_vec = g.c_ns == 1 and g.c % 16 == 0 and g.c_ms % 16 == 0 and g.c_bs % 16 == 0
            name += " | c_vec" + (", a partial last chunk" if g.N % 16 else "") if c_vec else " | byte stores"
        return name, []
    small = g.K <= 512 and g.batch * g.M * g.N * g.K <= (1 << 22)
    if g.K == 0 or (native and (small or (esz == 1 and not _longk_shape(g.M, g.K, g.N)))):
        return f"k_gemm_{'widen' if wide_out else 'narrow'}_generic<{GENERIC_T[dt]}>", []
    # plan_widened: both operands converted into contiguous row-major temporaries, the wide plan, the result converted back (not wide_out)
    pool = [g.ba * g.M * g.K * 4, g.bb * g.K * g.N * 4] + ([] if wide_out else [g.batch * g.M * g.N * 4])
    if esz == 1:                            # plan_gemm(int32): the long-k hand-off, else the generic kernel
        if _longk_shape(g.M, g.K, g.N):
            k, p = _longk_kernels("int", g.M, g.K, g.N, g.batch, 4)
            pool.append(p)
        else:
            k = "k_gemm_generic<int>"
    else:                                   # plan_gemm(float32): hand-offs, then plan_mfma on the forced 64 x 64 tile
        assert o["gemm_cfg"] == 1 and o["gemm_peel"] == 0, (e.id, "the widened float16 entries force the wide tile")
        assert not _skinny_floors(g) and wide_paths._skinny(f32, "NN", g.M, g.K, g.N, g.batch) is None, e.id
        if _longk_shape(g.M, g.K, g.N) and not (max(g.M, g.N) > 8 and min(g.M, g.N) >= 64):
            k, p = _longk_kernels("float", g.M, g.K, g.N, g.batch, 4)
        elif g.M * g.N < 4096 or g.K < 8:       # md_gemm_layout: too small for the MFMA kernels
            k, p = "k_gemm_generic<float>", 0
        else:                                   # (the temporaries' row steps are K and N: vec_ok wants multiples of four)
            aligned = g.K % 4 == 0 and g.N % 4 == 0 and (g.ba == 1 or g.M * g.K % 4 == 0) and (g.bb == 1 or g.K * g.N % 4 == 0)
            k, p = wide_paths._mfma_kernel(1, "NN", g.M, g.K, g.N, g.batch, aligned=aligned)
        pool.append(p)
    return f"{CONV} x2 + {k}" + ("" if wide_out else f" + {CONV}"), pool


# md_options.h defaults of everything an entry may set: put back before every entry (the interleaved tests run many in one test)
DEFAULTS = {"gemm_cfg": -1, "gemm_peel": 1, "gemm_widen": 1, "gemm_narrow_skinny": 1, "gemm_splitk": 1, "gemm_skinny": 1}
WIDE_TILE = {"gemm_cfg": 1, "gemm_peel": 0}      # what a float16 entry that may take the widened route sets


class Entry:
    def __init__(self, id, kind, M, K, N, batch=1, lay="NN", a=PLAIN, b=PLAIN, c="contig", opts=None, rep=False, public=False, note=""):
        self.id, self.kind, self.M, self.K, self.N, self.batch, self.lay = id, kind, M, K, N, batch, lay
        self.a, self.b, self.c, self.opts, self.rep, self.public = a, b, c, dict(opts or {}), rep, public
        self.dt, self.ct = KINDS[kind]
        self.flt = self.dt == f16
        self.work = batch * M * N * K
        self.route, pool = _route(self, _gemm(self))               # (for bases on a 16-B boundary: _run restates it from the real ones)
        self.reaches = self.route + (" | " + note if note else "")
        self.pool = tuple(int(p) for p in pool if p)

    @property
    def cpu(self):
        return self.work <= CPU_MAX

    @property
    def kernels(self):
        return self.reaches.split(" | ")[0].split(" + ")


TABLE = []


def _add(*a, **k):
    TABLE.append(Entry(*a, **k))
    return TABLE[-1]


def _bk(kind):
    return 128 // KINDS[kind][0].itemsize


def _epc(kind):
    return 16 // KINDS[kind][0].itemsize


def _opts(kind, **more):
    """float16 entries that the planner may send down the widened route force the wide plan's tile; harmless on every other route"""
    return {**(WIDE_TILE if KINDS[kind][0] == f16 else {}), **more}


# ---- 1. whole tiles, every k-tile count: the prologue alone, both exits of the two-way unrolled loop, a second trip -------------------------
for ki, kind in enumerate(KINDS):
    for li, lay in enumerate(LAYS):
        for kt in (1, 2, 3, 4, 5):
            _add(f"whole-{kind}-{lay}-kt{kt}", kind, 128, kt * _bk(kind), 256, lay=lay, c=C_ALL[(ki + li + kt) % 6], public=(kt == 3 and li == ki % 4))

# ---- 2. EDGE: each kind of raggedness on its own and together ---------------------------------------------------------------------------------
for ki, kind in enumerate(KINDS):
    bk, epc = _bk(kind), _epc(kind)
    for li, lay in enumerate(LAYS):
        a_kc, b_kc = lay[0] == "N", lay[1] == "T"
        rm, rn = (1 if a_kc else epc), (1 if b_kc else epc)        # a KC image takes any row count, an MN image whole chunks of rows
        c = lambda j: C_ALL[(ki + li + j) % 6]
        _add(f"edge-{kind}-{lay}-m", kind, 128 + rm, 2 * bk, 128, lay=lay, c=c(0))
        _add(f"edge-{kind}-{lay}-n", kind, 128, 2 * bk, 128 + rn, lay=lay, c=c(1))
        for kt in (1, 2):
            _add(f"edge-{kind}-{lay}-k{kt}", kind, 128, kt * bk + epc, 128, lay=lay, c=c(1 + kt))
        if lay == "TN":                                              # neither operand k-contiguous: any K
            _add(f"edge-{kind}-TN-k-odd", kind, 128, bk + 1, 128, lay=lay, c=c(4))
        # the smallest products the kernels take: 9 rows of a KC image (8 are thin), two chunks of an MN image; one chunk of k
        _add(f"edge-{kind}-{lay}-smallest", kind, 9 if a_kc else max(16, epc), epc, 9 if b_kc else max(16, epc), lay=lay, c=c(5))
        _add(f"edge-{kind}-{lay}-all", kind, 128 + rm, bk + (3 if lay == "TN" else epc), 256 - rn, lay=lay, c=c(6), public=(li == (ki + 1) % 4))

# ---- 3. the tile map: tile counts 1, 2, 3, 7, 8, 9, 10, 15, 17 at one k-tile — each tile written exactly once --------------------------------
MAP_SHAPES = [(1, n) for n in (1, 2, 3, 7, 8, 9, 10, 15, 17)] + [(n, 1) for n in (2, 3, 7, 8, 9, 10, 15, 17)] + [(3, 3), (5, 2)]
for kind in ("i8", "f16"):
    for si, (tm, tn) in enumerate(MAP_SHAPES + [(5, 2)]):
        batch = 3 if si == len(MAP_SHAPES) else 1
        tag = f"map-{kind}-{tm}x{tn}" + ("-batch3" if batch > 1 else "")
        _add(tag + "-whole", kind, TILE * tm, _bk(kind), TILE * tn, batch=batch, lay=LAYS[si % 4], c="bpad" if batch > 1 else "contig")
        _add(tag + "-edge", kind, TILE * tm - 5, _bk(kind), TILE * tn - 3, batch=batch, lay="NT", c="ms+1" if si % 2 else "contig")

# ---- 4. operands inside larger bases ---------------------------------------------------------------------------------------------------------
for ki, kind in enumerate(KINDS):
    bk, epc = _bk(kind), _epc(kind)
    for li, lay in enumerate(LAYS):
        # what md_narrow_layout accepts: the DMA address arithmetic of stage<> (whole tiles and EDGE alternate)
        for j, (tag, a, b, batch) in enumerate((
                ("pad1", Op(pad=epc), Op(pad=4 * epc), 1), ("pad4", Op(pad=4 * epc), Op(pad=epc), 1),
                ("off1", Op(off=epc), Op(off=3 * epc), 1), ("off3", Op(off=3 * epc, pad=epc), Op(off=epc), 1),
                ("bpad", Op(bpad=epc), Op(bpad=3 * epc, pad=epc), 2))):
            if (j + li + ki) % 2:
                _add(f"view-{kind}-{lay}-{tag}", kind, 128, 2 * bk, 256, batch=batch, lay=lay, a=a, b=b, c=C_ALL[(j + li) % 6])
            else:
                _add(f"view-{kind}-{lay}-{tag}-edge", kind, 128 + epc, bk + epc, 128 - epc, batch=batch, lay=lay, a=a, b=b, c=C_ALL[(j + li) % 6])
    # broadcasts over the batch: A (a_bs = 0); B folded into M by md_build_gemm; B with a padded C batch step (no fold)
    lay = LAYS[ki % 4]
    _add(f"view-{kind}-a-broadcast", kind, 128, 2 * bk, 128, batch=3, lay=lay, a=Op(one=True), c="bpad")
    _add(f"view-{kind}-b-broadcast-folded", kind, 128, bk, 128, batch=3, lay="N" + lay[1], b=Op(one=True), note="md_build_gemm folds the batch into M")
    _add(f"view-{kind}-b-broadcast-folded-edge", kind, 72, bk + epc, 128, batch=3, lay="N" + lay[1], b=Op(one=True), note="md_build_gemm folds the batch into M")
    _add(f"view-{kind}-b-broadcast-padded-c", kind, 128, bk, 128, batch=3, lay=lay, b=Op(one=True, pad=epc), c="bpad")
    # every reason md_narrow_layout has to refuse, once per operand (the layout puts the image in question on that operand)
    for who in ("a", "b"):
        kc_lay, mn_lay = ("NN", "TN") if who == "a" else ("TT", "TN")      # the operand as a KC / an MN image, the other one taken
        for tag, lay, op, dims, batch in (
                ("start-1", kc_lay, Op(off=1), (128, bk, 128), 1), ("row-step", mn_lay, Op(pad=1), (128, bk, 128), 1),
                ("batch-step", kc_lay, Op(bpad=1), (64, bk, 64), 2), ("k-chunk", kc_lay, PLAIN, (128, bk + 1, 128), 1),
                ("rows-chunk", mn_lay, PLAIN, (128 + (who == "a"), bk, 128 + (who == "b")), 1),
                ("step2", kc_lay, Op(kind="step2"), (128, bk, 128), 1), ("flip", mn_lay, Op(kind="flip"), (128, bk, 128), 1),
                ("bcast", kc_lay, Op(kind="bcast"), (128, bk, 128), 1)):
            M, K, N = dims
            _add(f"refused-{kind}-{who}-{tag}", kind, M, K, N, batch=batch, lay=lay, a=op if who == "a" else PLAIN, b=op if who == "b" else PLAIN,
                 c=C_ALL[(ki + len(tag)) % 6], opts=_opts(kind), note=f"md_narrow_layout refuses {who}")

# ---- 5. C layouts: each against each output type, whole and EDGE; the int8 / uint8 write-out's arms -------------------------------------------
for ki, kind in enumerate(KINDS):
    for ci, c in enumerate(C_ALL):
        batch = 2 if c == "bpad" else 1
        _add(f"c-{kind}-{c}-whole", kind, 128, _bk(kind), 256, batch=batch, lay=LAYS[(ki + ci) % 4], c=c)
        _add(f"c-{kind}-{c}-edge", kind, 100, _bk(kind), 130, batch=batch, lay="NT", c=c)
for kind in ("i8", "u8"):
    _add(f"c-{kind}-vec-n-chunks", kind, 130, 128, 144, lay="NT", c="ms+16B", public=True)
    _add(f"c-{kind}-vec-partial-chunk", kind, 130, 128, 128 + 2, lay="NT", c="ms+16B")
    _add(f"c-{kind}-vec-chunk-less-one", kind, 130, 128, 128 + 15, lay="NT", c="ms+16B")       # (n + 16 = N + 1: the closest a byte-loop chunk gets)
    _add(f"c-{kind}-vec-chunk-less-one-batch", kind, 64, 128, 256 + 15, batch=2, lay="NT", c="ms+16B")

# ---- 6. the generic kernels -------------------------------------------------------------------------------------------------------------------
ODD3 = Op(pad=1, off=1, bpad=1)
for kind in KINDS:
    o = _opts(kind)
    _add(f"generic-{kind}-tiny", kind, 3, 5, 7, c="ms+1", opts=o, public=True)
    _add(f"generic-{kind}-k0", kind, 33, 0, 17, c="off1", opts=o, note="K = 0: C all zero")
    for K in (15, 16, 17):
        _add(f"generic-{kind}-k{K}", kind, 33, K, 29, lay=LAYS[K % 4], a=Op(off=1), c=C_ALL[K % 6], opts=o)
    _add(f"generic-{kind}-step2", kind, 40, 24, 50, lay="NN", a=Op(kind="step2"), b=Op(kind="step2"), opts=o)
    _add(f"generic-{kind}-flip", kind, 35, 33, 45, lay="NT", a=Op(kind="flip"), b=Op(kind="flip"), c="T", opts=o)
    _add(f"generic-{kind}-bcast", kind, 40, 33, 50, lay="TN", a=Op(kind="bcast"), b=Op(kind="bcast"), c="ms+1", opts=o)
    _add(f"generic-{kind}-batch3-odd-strides", kind, 17, 19, 33, batch=3, lay="TT", a=ODD3, b=ODD3, c="off1", opts=o)
    _add(f"generic-{kind}-batch3-b-broadcast", kind, 17, 19, 33, batch=3, lay="NN", a=ODD3, b=Op(one=True, off=1), c="ms+1", opts=o)
for kind in ("f16->f32", "i8->i32"):
    _add(f"generic-{kind}-k0-widen-off", kind, 20, 0, 20, opts=_opts(kind, gemm_widen=0), note="K = 0 under gemm_widen = 0")

# ---- 7. the widened route -----------------------------------------------------------------------------------------------------------------------
def _few_long_cut(blocks):
    """the smallest whole number of float16 k-tiles that is few_long for `blocks` tiles"""
    kt = 1
    while not _few_long(64 * kt, blocks):
        kt += 1
    return 64 * kt


for kind in ("f16", "f16->f32"):
    o = _opts(kind)
    # refused by the layout and not small
    _add(f"widened-{kind}-k520-start-1", kind, 128, 520, 128, a=Op(off=1), c="ms+1", opts=o, public=True)
    _add(f"widened-{kind}-k512-over-2^22", kind, 128, 512, 65, lay="NT", b=Op(off=1), c="T", opts=o)
    _add(f"widened-{kind}-batch2-a-broadcast", kind, 96, 520, 80, batch=2, lay="TN", a=Op(one=True, pad=1), b=Op(bpad=8), c="bpad", opts=o)
    # negative and zero strides: S_NCONV sees them
    _add(f"widened-{kind}-flip", kind, 128, 520, 72, lay="NN", a=Op(kind="flip"), b=Op(kind="flip"), c="off1", opts=o)
    _add(f"widened-{kind}-bcast-step2", kind, 72, 528, 128, lay="NT", a=Op(kind="bcast"), b=Op(kind="step2"), opts=o)
    # few_long on each side of its cut, 1 and 4 tiles (K in the thousands: {-1, 1} data); past the cut the wide plan splits k
    for tiles, (M, N) in ((1, (128, 128)), (4, (256, 256))):
        K = _few_long_cut(tiles)
        _add(f"widened-{kind}-few-long-{tiles}-tiles", kind, M, K, N, lay=LAYS[tiles % 4], c="ms+16B", opts=o, rep=True, note=f"few_long from K = {K}")
        _add(f"widened-{kind}-not-yet-few-long-{tiles}-tiles", kind, M, K - 64, N, lay=LAYS[tiles % 4], c="ms+16B", opts=o, rep=(tiles == 1),
             note=f"few_long from K = {K}")
# gemm_widen = 0: every wide-output product with a k converts its operands and runs the wide plan straight into C
for c in ("contig", "ms+1", "T"):
    _add(f"widened-f16->f32-widen-off-{c}", "f16->f32", 128, 128, 256, lay="NT", c=c, opts=_opts("f16->f32", gemm_widen=0))
    _add(f"widened-i8->i32-widen-off-{c}", "i8->i32", 128, 128, 256, lay="NT", c=c, opts={"gemm_widen": 0})
_add("widened-f16->f32-widen-off-k1024", "f16->f32", 64, 1024, 64, lay="TN", c="ms+16B", opts=_opts("f16->f32", gemm_widen=0), rep=True)
_add("widened-f16->f32-widen-off-tiny", "f16->f32", 3, 5, 7, opts=_opts("f16->f32", gemm_widen=0))
_add("widened-i8->i32-widen-off-longk", "i8->i32", 5, 4097, 7, lay="NT", c="ms+1", opts={"gemm_widen": 0})
# int8 / uint8 at a long-k shape without the hand-off: the conversion, the int32 long-k kernels, the conversion back
for kind in ("i8", "u8", "i8->i32"):
    _add(f"widened-{kind}-longk-16x8192x16", kind, 16, 8192, 16, lay="TN", c="ms+1", opts={"gemm_narrow_skinny": 0})
    _add(f"widened-{kind}-longk-5x600x7", kind, 5, 600, 7, batch=2, lay="NT", a=Op(kind="flip"), b=Op(one=True, kind="bcast"), c="bpad", opts={"gemm_narrow_skinny": 0})

# ---- 8. the cuts of plan_narrow_declined, one entry on each side ----------------------------------------------------------------------------
for kind in KINDS:
    o, bk = _opts(kind), _bk(kind)
    # thin: min(M, N) = 8 / 9, below the hand-off's floors (R < 512), in both orientations
    for n in (8, 9):
        _add(f"cut-{kind}-thin-m{n}", kind, n, 2 * bk, 256, lay="NT", c="ms+1", opts=o)
        _add(f"cut-{kind}-thin-n{n}", kind, 256, 2 * bk, n, lay="NT", c="T", opts=o)
    _add(f"cut-{kind}-thin-m8-k576", kind, 8, 576, 136, lay="NT", opts=o, note="thin and K > 512")
    # small: refused by the layout (a start one element in), K = 512 / 520 and batch M N K = 2^22 / just over
    _add(f"cut-{kind}-small-k512", kind, 128, 512, 64, a=Op(off=1), opts=o)
    _add(f"cut-{kind}-small-k520", kind, 64, 520, 64, a=Op(off=1), opts=o)
    _add(f"cut-{kind}-small-over-2^22", kind, 129, 512, 64, a=Op(off=1), opts=o)
for kind in ("i8", "u8", "i8->i32"):
    # md_longk_shape for one-byte operands: K = 8192 is the hand-off's (without it: the widened route), K = 8191 the MFMA kernel's
    _add(f"cut-{kind}-longk-k8192", kind, 16, 8192, 16, lay="TN", c="ms+1")
    _add(f"cut-{kind}-longk-k8191", kind, 16, 8191, 16, lay="TN", c="ms+1")
    _add(f"cut-{kind}-longk-k8191-handoff-off", kind, 16, 8191, 16, lay="TN", c="ms+1", opts={"gemm_narrow_skinny": 0})
    _add(f"cut-{kind}-longk-m144", kind, 144, 9216, 16, lay="TN", opts={"gemm_narrow_skinny": 0}, note="M > 128: no long-k shape")

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE), [e.id for e in TABLE if sum(x.id == e.id for x in TABLE) > 1]
IDS = [e.id for e in TABLE]


# ---- what the table must cover -------------------------------------------------------------------------------------------------------------
def test_table_names_every_instantiation():
    names = {k for e in TABLE for k in e.kernels}
    bools = ("true", "false")
    want = {f"k_gemm_{f}_mfma<{esz}, {a}, {b}, {edge}>" for f in ("narrow", "widen") for esz in (2, 1) for a in bools for b in bools for edge in bools}
    want |= {f"k_gemm_narrow_generic<{t}>" for t in GENERIC_T.values()} | {f"k_gemm_widen_generic<{GENERIC_T[t]}>" for t in (f16, i8)}
    assert len(want) == 37 and not want - names, sorted(want - names)
    for lay in LAYS:        # uint8 on the ESZ = 1 kernels in every layout, whole and EDGE
        for edge in bools:
            k = f"k_gemm_narrow_mfma<1, {_b(lay[0] == 'N')}, {_b(lay[1] == 'T')}, {edge}>"
            assert any(e.kind == "u8" and e.lay == lay and e.kernels == [k] for e in TABLE), (lay, edge)
    # the write-out arms of the int8 kernel, and both routes on each side of every cut
    for kind in ("i8", "u8"):
        notes = {e.route.split(" | ")[1] for e in TABLE if e.kind == kind and e.kernels[0].startswith("k_gemm_narrow_mfma")}
        assert notes >= {"c_vec", "c_vec, a partial last chunk", "byte stores"}, (kind, notes)
    assert any(CONV in e.reaches and "k_gemm_splitk_sum" in e.reaches for e in TABLE) and any("k_longk_partial<int" in e.reaches for e in TABLE)
    # the views md_narrow_layout accepts reach the MFMA kernels, the ones it refuses do not; each cut has both routes
    for e in TABLE:
        sec = e.id.split("-")[0]
        assert sec not in ("whole", "edge", "map", "view", "c") or "_mfma<" in e.kernels[0], (e.id, e.reaches)
        assert sec not in ("refused", "generic", "widened") or "_mfma<" not in e.kernels[0] or "not-yet" in e.id, (e.id, e.reaches)
        assert sec != "widened" or "not-yet" in e.id or e.kernels[0] == CONV + " x2", (e.id, e.reaches)
    for kind in KINDS:
        for cut in ("thin-m", "thin-n", "small"):
            routes = {e.kernels[0] for e in TABLE if e.id.startswith(f"cut-{kind}-{cut}")}
            assert len(routes) >= 2 or (cut == "small" and KINDS[kind][0] != f16), (kind, cut, routes)


def test_table_keeps_to_the_size_rule():
    """No entry but the tile map's is longer than three tiles on a side or five k-tiles on the MFMA kernels; K in the thousands only on the
    few_long and long-k entries; every section has a CPU half."""
    sections = {}
    for e in TABLE:
        sec = e.id.split("-")[0]
        sections.setdefault(sec, []).append(e.cpu)
        if sec != "map":
            assert max(e.M, e.N) <= 3 * TILE, e.id
        if "_mfma<" in e.kernels[0] and "few-long" not in e.id and "longk" not in e.id:
            assert e.K <= 5 * _bk(e.kind) + _epc(e.kind), e.id
        if e.K >= 1024:
            assert "few-long" in e.id or "longk" in e.id or e.id == "widened-f16->f32-widen-off-k1024", e.id
    assert all(any(v) for v in sections.values()), {k: any(v) for k, v in sections.items()}


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("MDHIP_NARROW_PATHS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float16 products of tests/test_narrow_matmul_paths.py: largest |got - exact| / (ulp(exact) / 2 + K 2^-23 (|a| @ |b|)) per path "
                    "(bound: 1)\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key]:8.5f}  {key}\n")


def _rng(e, salt):
    return np.random.default_rng([IDS.index(e.id) if e.id in BY_ID else len(IDS), salt])


def _filler(dt, n, rng):
    if dt.kind == "f":
        return np.full(n, np.nan, dtype=dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def _place(x, trans, op, rng):
    """The logical (B, R, C) operand inside its base: -> (flat base, offset, element strides of the logical axes)."""
    st = x.transpose(0, 2, 1) if trans else x
    B, rows, cols = st.shape
    n, off, (bs, rs, cs) = _geometry(rows, cols, B, op, 16 // x.dtype.itemsize)
    flat = _filler(x.dtype, n, rng)
    idx = off + np.arange(B)[:, None, None] * bs + np.arange(rows)[None, :, None] * rs + np.arange(cols)[None, None, :] * cs
    flat[idx] = st
    return flat, off, ((bs, cs, rs) if trans else (bs, rs, cs))


def _operands(e, A, B, rng):
    """Device views of A (batch or 1, M, K) and B (batch or 1, K, N) in the entry's layout (the bases stay alive with the views)."""
    out = []
    for x, trans, op in ((A, e.lay[0] == "T", e.a), (B, e.lay[1] == "T", e.b)):
        flat, off, strides = _place(x, trans, op, rng)
        base = nd.asarray(flat)
        out.append((base._view(off, x.shape, strides), base))
    return out


def _logical(e, A, B):
    """What the views hold: stride 0 across the stored rows repeats the first stored row, a single batch is the first one."""
    if e.a.kind == "bcast":
        A = np.ascontiguousarray(np.broadcast_to(A[:, :, :1] if e.lay[0] == "T" else A[:, :1, :], A.shape))
    if e.b.kind == "bcast":
        B = np.ascontiguousarray(np.broadcast_to(B[:, :, :1] if e.lay[1] == "T" else B[:, :1, :], B.shape))
    return (A[:1] if e.a.one else A), (B[:1] if e.b.one else B)


def _poison_pool(e):
    """Blocks of the byte sizes the plan's temporaries take, full of NaN, back on the free lists."""
    blocks = [nd.asarray(np.full(n // 4, np.nan, dtype=f32)) for n in e.pool]      # (all live at once: distinct blocks)
    del blocks


SENTINEL = 0xA5
PUBLIC_FORMS = ("plain", "out", "dtype")      # (the wide-output kinds pass `dtype=` in every form: "dtype" is the others' third)


def _run(e, A, B, rng, on_gpu, via_public=None):
    """C = A @ B of the entry through the C-ABI into a sentinel-filled base -> the view's values (surroundings checked)."""
    (da, base_a), (db, base_b) = _operands(e, A, B, rng)
    kw = {"dtype": e.ct} if e.ct != e.dt or via_public == "dtype" else {}
    if via_public == "out":
        out = nd.asarray(np.full((e.batch, e.M, e.N), SENTINEL, dtype=np.uint8).astype(e.ct))
        r = nd.matmul(da, db, out=out, **kw)
        assert r is out
        return out.get()
    if via_public:
        return nd.matmul(da, db, **kw).get()
    off, bs, ms, ns = C_LAYOUTS[e.c](e.M, e.N, 16 // e.ct.itemsize)
    n = off + e.batch * bs + 16
    base = nd.asarray(np.full(n * e.ct.itemsize, SENTINEL, dtype=np.uint8).view(e.ct))
    dc = base._view(off, (e.batch, e.M, e.N), (bs, ms, ns))
    ad, bd, cd = da.desc(), db.desc(), dc.desc()
    if on_gpu:          # the route from the real byte addresses of the bases: the table assumed 16-B aligned ones
        real = _route(e, _gemm(e, ad.data - da._offset * e.dt.itemsize, bd.data - db._offset * e.dt.itemsize, cd.data - off * e.ct.itemsize))[0]
        assert real == e.route, (e.id, real, e.route)
    _poison_pool(e)
    nd._lib().matmul(ad, bd, cd)
    flat = base.get()
    idx = off + np.arange(e.batch)[:, None, None] * bs + np.arange(e.M)[None, :, None] * ms + np.arange(e.N)[None, None, :] * ns
    outside = np.ones(n, dtype=bool)
    outside[idx] = False
    assert (flat.view(np.uint8).reshape(n, -1)[outside] == SENTINEL).all(), (e.id, "bytes of C's base outside the view were written")
    return flat[idx]


def _exact_data(e, rng):
    shape_a, shape_b = (e.batch, e.M, e.K), (e.batch, e.K, e.N)
    if e.dt == f16:
        vals = np.array([-1, 1] if e.K >= 1024 else [-3, -1, 1, 3], dtype=f16)
        A, B = _logical(e, rng.choice(vals, shape_a), rng.choice(vals, shape_b))
        ref = np.matmul(A.astype(np.float64), B.astype(np.float64))      # exact: odd integers, every partial sum below 2^24
        assert (ref % 2 == e.K % 2).all() and np.matmul(np.abs(A.astype(np.float64)), np.abs(B.astype(np.float64))).max(initial=0) < 2 ** 24
        if e.ct == f16:
            assert np.abs(ref).max(initial=0) <= 2048, (e.id, "the data's precondition: the cast to float16 is exact")
        return A, B, ref.astype(e.ct)
    info = np.iinfo(e.dt)
    A, B = (rng.integers(info.min, info.max, s, dtype=e.dt, endpoint=True) for s in (shape_a, shape_b))
    for x in (A, B):                                                      # the extremes, wherever the random bytes missed them
        x.reshape(-1)[:4] = np.array([info.min, info.max, info.max, info.min], dtype=e.dt)[:x.size]
    A, B = _logical(e, A, B)
    ref = np.matmul(A.astype(np.float64), B.astype(np.float64))          # exact: |sum| <= 2^16 K < 2^53
    return A, B, np.broadcast_to(np.rint(ref).astype(np.int64).astype(e.ct), (e.batch, e.M, e.N))


def _float_data(e, rng):
    A, B = rng.standard_normal((e.batch, e.M, e.K)).astype(f16), rng.standard_normal((e.batch, e.K, e.N)).astype(f16)
    return _logical(e, A, B)


def _set_opts(e, mdopt, extra=None):
    for k, v in {**DEFAULTS, **e.opts, **(extra or {})}.items():
        mdopt(k, v)


def _fma_chain(A, B, ct):
    """The generic kernels' claim: a float32 accumulator over k = 0 .. K-1 of the (exact) float32 products, one cast at the end."""
    a, b = A.astype(f32), B.astype(f32)
    acc = np.zeros(np.broadcast_shapes(a.shape[:1], b.shape[:1]) + (a.shape[1], b.shape[2]), dtype=f32)
    for k in range(a.shape[2]):
        acc = acc + a[:, :, k, None] * b[:, k, None, :]
    return acc.astype(ct)


def _float_check(e, A, B, got, extra=""):
    """The contract of tests/test_narrow_thin.py::_check; the largest error / bound is recorded per `reaches`."""
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    exact, mag = np.matmul(a64, b64), np.matmul(np.abs(a64), np.abs(b64))
    assert got.dtype == e.ct and got.shape == exact.shape
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(exact).astype(e.ct)).astype(np.float64)
    fin = np.isfinite(ulp)
    assert np.array_equal(np.isfinite(got), fin), (e.id, "finite where the reference is")
    bound = ulp / 2 + e.K * 2.0 ** -23 * mag
    ratio = float((np.abs(got.astype(np.float64) - exact)[fin] / bound[fin]).max(initial=0.0))
    key = e.reaches + extra
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    assert ratio <= 1.0, (e.id, ratio)
    if "_generic<_Float16" in e.kernels[0]:
        want = _fma_chain(A, B, e.ct)
        diff = int((got.view(np.uint8) != want.view(np.uint8)).any(axis=-1).sum()) if got.size else 0
        assert diff == 0, (e.id, f"{diff} of {got.size} outputs differ from the float32 fma chain in k order")


def _check_entry(e, mdopt, on_gpu, via_public=None):
    if not on_gpu and not e.cpu:
        pytest.skip("batch M N K > 2^24: the CPU double is a triple loop")
    _set_opts(e, mdopt)
    A, B, ref = _exact_data(e, _rng(e, 1))
    got = _run(e, A, B, _rng(e, 2), on_gpu, via_public)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref, err_msg=f"{e.id}: {e.reaches}")
    if e.flt:
        A, B = _float_data(e, _rng(e, 3))
        _float_check(e, A, B, _run(e, A, B, _rng(e, 4), on_gpu, via_public), " public" if via_public else "")


@_twins(IDS)
def _kernel_paths(case, mdopt, on_gpu):
    _check_entry(BY_ID[case], mdopt, on_gpu)


test_kernel_paths, test_kernel_paths_gpu = _kernel_paths

PUBLIC = [f"{e.id}:{form}" for e in TABLE if e.public for form in PUBLIC_FORMS if form != "dtype" or e.ct == e.dt]


@_twins(PUBLIC)
def _public_functions(case, mdopt, on_gpu):
    """A subset through nd.matmul on the same operand views: a fresh C-contiguous result, `out=` pre-filled with a wrong value, and
    `dtype=` — the operands' own type, or the wide one (float16 -> float32, int8 -> int32: the wide-output kinds, in every form)."""
    id_, form = case.rsplit(":", 1)
    _check_entry(BY_ID[id_], mdopt, on_gpu, via_public=form)


test_public_functions, test_public_functions_gpu = _public_functions


# ---- bit identity ------------------------------------------------------------------------------------------------------------------------------
@_twins([f"{kind}:kt{kt}" for kind in ("f16", "f16->f32") for kt in (2, 3)])
def _layouts_and_edge_give_the_same_bits(case, mdopt, on_gpu):
    """One float16 product of whole tiles on float data: NN, NT, TN and TT run the same sums in the same order (the KC read and the
    transposed reads hand the same k to element j of a lane), and so does the EDGE kernel on a problem one chunk larger in M and N whose
    top-left tiles are this product."""
    kind, kt = case.split(":kt")[0], int(case.split(":kt")[1])
    M, K, N, epc = 128, kt * 64, 256, 8
    rng = np.random.default_rng([len(IDS), 21, kt])
    A, B = rng.standard_normal((1, M + epc, K)).astype(f16), rng.standard_normal((1, K, N + epc)).astype(f16)
    first = None
    for lay in LAYS:
        for grow in (0, epc):
            e = Entry(f"identity-{kind}-{lay}-kt{kt}-{'edge' if grow else 'whole'}", kind, M + grow, K, N + grow, lay=lay, c="ms+16B")
            assert e.kernels == [f"k_gemm_{'widen' if kind != 'f16' else 'narrow'}_mfma<2, {_b(lay[0] == 'N')}, {_b(lay[1] == 'T')}, {_b(grow)}>"]
            _set_opts(e, mdopt)
            a, b = np.ascontiguousarray(A[:, :M + grow]), np.ascontiguousarray(B[:, :, :N + grow])
            got = _run(e, a, b, np.random.default_rng(5), on_gpu)
            _float_check(e, a, b, got)
            bits = np.ascontiguousarray(got[:, :M, :N]).view(np.uint8)
            if first is None:
                first = bits
            diff = int((bits != first).sum())
            assert diff == 0, (e.id, f"{diff} of {bits.size} bytes differ from the whole-tile NN product")


test_layouts_and_edge_give_the_same_bits, test_layouts_and_edge_give_the_same_bits_gpu = _layouts_and_edge_give_the_same_bits

REPEATED = [e.id for e in TABLE if e.rep] + ["whole-f16-TN-kt3", "edge-f16->f32-NT-all", "map-f16-3x3-whole"]


@_twins(["repeats"])
def _repeats_give_the_same_bits(case, mdopt, on_gpu):
    """The widened entries whose wide plan splits k (partials from the pool, k_gemm_splitk_sum) and three MFMA entries, three times
    interleaved with each other, the pool poisoned before every call: each repeat must give the bits of the first."""
    ids = REPEATED if on_gpu else [i for i in REPEATED if BY_ID[i].cpu]
    assert sum("k_gemm_splitk_sum" in BY_ID[i].reaches for i in REPEATED) >= 4 and len(ids) >= 4
    runs = []
    for id_ in ids:
        e = BY_ID[id_]
        A, B = _float_data(e, _rng(e, 6))
        runs.append((e, A, B))
    first = {}
    for order in (range(len(runs)), range(len(runs) - 1, -1, -1), range(len(runs))):
        for k in order:
            e, A, B = runs[k]
            _set_opts(e, mdopt)
            got = _run(e, A, B, _rng(e, 7), on_gpu).tobytes()
            assert first.setdefault(k, got) == got, (e.id, e.reaches)


test_repeats_give_the_same_bits, test_repeats_give_the_same_bits_gpu = _repeats_give_the_same_bits
