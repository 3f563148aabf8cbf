"""Every launch form of the float32 / float64 / integer matmul (csrc/gemm.hip, csrc/skinny.hip) against exact references.

The centre is TABLE: what an entry reaches (kernel names with their template arguments, as a kernel trace prints them), the
dtype, M, K, N, batch, the layout of A and B ("NN" .. "TT": which of them is stored transposed), how A, B and C sit in their base
arrays, and the options set through the `mdopt` fixture. There is no hook that reports which kernel ran: `reaches` is derived
per entry by _mfma_kernel & co., which restate the planner's predicates (plan_gemm -> plan_kranges / plan_f32 -> plan_peeled ->
plan_mfma, plan_f64, md_gemm_skinny, md_gemm_longk; MD_NUM_CUS 256), and is to be confirmed by a kernel trace of the gpu half
(profiles/README.md: matmul_paths_kernel_stats.csv). Tiles are forced with option gemm_cfg, so one to three tiles per side do.
The calls go through the C-ABI (lib.matmul on descriptors): that is what takes a strided C. test_public_functions runs a subset
through nd.matmul, `out=` included.

What every entry checks:
  exact data     operands from the ODD values {-3, -1, 1, 3}: every k-term is odd, so one dropped or doubled term flips the
                 parity of an output; every partial sum in any order is an exact integer (9 K < 2^24 for every K here), so the
                 result equals the float64 product of the same values (exact: < 2^53), compared with array_equal. int32 /
                 int64: full-range random values, the result must equal NumPy's wrapping product of the same dtype.
  surroundings   A, B and C are views of larger bases. Float padding of A and B is NaN (integers: random): a lane that reads
                 past its operand and lets it reach C fails the exact check. Every byte of C's base, view included, is 0xA5
                 before the call: afterwards the view equals the reference and every byte outside it is still 0xA5.
  the pool       before a call whose plan takes temporaries (split-K / k-range partials, repack buffers, colsum planes, long-k
                 block partials) blocks of exactly those byte sizes are allocated, filled with NaN and freed, so that the
                 allocator's free lists hand THEM out: a form that reads a partial it never wrote reads NaN. The sizes are
                 computed per entry from the launchers' formulas (`pool`).
  float data     standard normals against float64 (float64 entries: np.longdouble):
                 |got - ref| <= 1.01 K u (|a| @ |b|) elementwise, u = 2^-24 / 2^-53 — the worst case of ANY summation order of
                 a K-term dot product (Higham, Accuracy and Stability, 3.5: gamma_K), so it is derived, not measured; 1.01
                 covers gamma_K = K u / (1 - K u). The largest error / bound per `reaches` goes to the file
                 MDHIP_MATMUL_PATHS_REPORT names (profiles/matmul_paths_error.txt holds the device run's).
Bit-identity: GROUPS lists option settings whose results on the same float data must equal the first member's bit for bit
(DESIGN.md says which forms share one k-ascending chain and which do not); the forms that change the order of summation
(split-K, k ranges, peel, skinny, long-k) are run three times interleaved with each other and must repeat their bits — a ticket
counter left off zero or a partial read from another launch would show.
The fused epilogue mdhip_matmul_bias_relu_sum is called directly (EPI, EPI_REFUSALS): exact mask and sum on integer data, the mask
of float data against the library's own plain product bit for bit, and a cancel check — identical rows of `a`, bias = -(row of
the plain product) — that is all-False / 0 if and only if the epilogue's accumulators carry the plain product's bits.
Mutation check (on scratch builds, not kept): each of (1) returning early from the last tile row of every super_h band, (2)
ending the NBUF = 3 loops one k-tile early, (3) storing the peeled right strip at n0 = 0 fails exactly the entries that name the
form — the super* entries and the k ranges; every NBUF = 3 entry; the peel entries with a right strip — by the sentinel left in
C, by the exact products, or by both.

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound; entries with batch M N K <= 2^24 only: the double
is a triple loop) — it proves data and references right — and gpu-marked on the product library."""
import os

import numpy as np
import pytest

from minidiff_amd import ndarray as nd

f32, f64, i32, i64 = np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.int64)
CUS = 256
CPU_MAX = 1 << 24

# ---- the tiles (gemm.hip kTiles): per cfg the register-staged tile and the direct-to-LDS tile, [0] NN / NT / TT, [1] TN -----------
T128, T64, T128x64, T256x128 = (128, 128, 16, 2, 2), (64, 64, 16, 2, 2), (128, 64, 16, 2, 2), (256, 128, 16, 2, 2)
D256, D128, D128x64, W8, W8R = (256, 256, 32, 2, 2), (128, 128, 32, 2, 2), (128, 64, 32, 2, 2), (128, 128, 32, 2, 4), (128, 128, 16, 2, 4)
REG = {0: (T128, T128), 1: (T64, T64), 2: (T128x64, T128x64), 3: (T256x128, T256x128), 4: (T256x128, D256), 5: (T128, D128),
       6: (T128x64, D128x64), 7: (W8R, W8)}
DMA = {0: (D128, None), 1: (None, None), 2: (None, None), 3: (None, None), 4: (D256, D256), 5: (D128, D128), 6: (None, D128x64), 7: (W8, W8)}


def _b(x):
    return "true" if x else "false"


def _kc(t, b_kc, ragged=0, nbuf=2, ct=False, epi=0):
    return f"k_gemm_f32_kc_glds<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, {_b(b_kc)}, {epi}, {ragged}, {nbuf}, {_b(ct)}>"


def _tn(t, ragged=0, nbuf=2):
    return f"k_gemm_f32_tn_glds<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, {ragged}, {nbuf}>"


def _reg(t, a_kc, b_kc, edge, splitk=False, epi=0):
    sched = 0 if (edge or splitk or t[0] == 64) else 1
    return f"k_gemm_f32_mfma<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, {_b(a_kc)}, {_b(b_kc)}, {_b(edge)}, {_b(splitk)}, {sched}, {epi}>"


def _lds3(t):
    return 3 * (t[0] + t[1]) * t[2] * 4 <= 128 * 1024


def _nbuf3(blocks, K, bk, forced):
    if K < 2 * bk:
        return False
    return forced == 3 if forced else blocks <= CUS


def _splitk(M, K, N, batch):
    """plan_mfma's split count on the 64 x 64 tile -> (splits, k_chunk)."""
    tiles = -(-M // 64) * -(-N // 64) * batch
    splits = min(-(-2 * CUS // tiles), K // 512, 256)
    if tiles >= CUS or K < 1024 or splits <= 1:
        return 1, K
    chunk = -(-(-(-K // splits)) // 16) * 16
    return -(-K // chunk), chunk


def _mfma_kernel(cfg, lay, M, K, N, batch=1, glds=1, nbuf=0, aligned=True, ct=False, pad_m=False, pad_n=False, splitk=1):
    """plan_mfma restated for operands with unit vector strides: -> (kernel names, bytes of the split-K partials or 0)."""
    a_kc, b_kc, tn = lay in ("NN", "NT"), lay in ("NT", "TT"), lay == "TN"
    family = bool(glds) and (a_kc or not b_kc)
    whole = (K % 4 == 0 if (a_kc or b_kc) else True) and (a_kc or M % 4 == 0 or pad_m) and (b_kc or N % 4 == 0 or pad_n)
    d = DMA[cfg][0]
    if a_kc and aligned and family and whole and d:
        ragged = bool(M % d[0] or N % d[1] or K % d[2])
        if not ragged or b_kc or N % 4 == 0:
            if ragged:
                return _kc(d, b_kc, 2 if (K % d[2] == 0 and d[0] <= 128) else 1), 0
            blocks = -(-M // d[0]) * -(-N // d[1]) * batch
            return _kc(d, b_kc, 0, 3 if _lds3(d) and _nbuf3(blocks, K, d[2], nbuf) else 2, ct and not b_kc), 0
    t = REG[cfg][1 if tn else 0]
    tiles = -(-M // t[0]) * -(-N // t[1]) * batch
    edge = bool(not aligned or M % t[0] or N % t[1] or K % t[2])
    if splitk and t[0] == 64 and t[1] == 64:
        splits, chunk = _splitk(M, K, N, batch)
        if splits > 1:
            edge = bool(edge or chunk % 16 or K % chunk % 16)
            return _reg(t, a_kc, b_kc, edge, True) + " + k_gemm_splitk_sum", splits * batch * M * N * 4
    if tn and DMA[cfg][1]:
        if edge:
            if aligned and family and whole:
                return _tn(t, 2 if (K % t[2] == 0 and t[0] <= 128) else 1), 0
        elif family:
            return _tn(t, 0, 3 if _lds3(t) and _nbuf3(tiles, K, t[2], nbuf) else 2), 0
    return _reg(t, a_kc, b_kc, edge), 0


def _ceil4(n):
    return (n + 3) // 4 * 4


class Op:
    """How an operand sits in its base: `pad` extra elements per stored row (the row length is first rounded up to 4), `off`
    elements in front of it, `bpad` extra elements per batch; kind: None | "step2" (every other stored column: both strides
    non-unit) | "flip" (negative stride along the stored columns) | "bcast" (stride 0 across the stored rows)."""
    def __init__(self, pad=0, off=0, bpad=0, kind=None):
        self.pad, self.off, self.bpad, self.kind = pad, off, bpad, kind

    @property
    def aligned(self):
        return self.pad % 4 == 0 and self.off % 4 == 0 and self.bpad % 4 == 0 and self.kind is None


PLAIN = Op()
# C layouts -> (offset, c_bs, c_ms, c_ns) in elements
C_LAYOUTS = {
    "contig": lambda M, N: (0, M * N, N, 1),
    "ms+4": lambda M, N: (0, M * (N + 4), N + 4, 1),
    "ms+1": lambda M, N: (0, M * (N + 1), N + 1, 1),
    "off1": lambda M, N: (1, M * N, N, 1),
    "T": lambda M, N: (0, N * (M + 4), 1, M + 4),
    "Toff1": lambda M, N: (1, N * (M + 4), 1, M + 4),
    "bpad": lambda M, N: (0, M * N + 8, N, 1),
    "bpad2": lambda M, N: (0, M * N + 2, N, 1),
}
C_ALL = ("contig", "ms+4", "ms+1", "off1", "T", "bpad")


class Entry:
    def __init__(self, id, reaches, dt, M, K, N, batch=1, lay="NN", a=PLAIN, b=PLAIN, c="contig", opts=None, pool=(), flt=None,
                 rep=False, public=False):
        self.id, self.reaches, self.dt, self.M, self.K, self.N, self.batch, self.lay = id, reaches, dt, M, K, N, batch, lay
        self.a, self.b, self.c, self.opts, self.pool = a, b, c, dict(opts or {}), tuple(int(p) for p in pool if p)
        self.flt = (dt.kind == "f") if flt is None else flt
        self.rep, self.public = rep, public
        self.work = batch * M * N * K

    @property
    def cpu(self):
        return self.work <= CPU_MAX


TABLE = []


def _add(*a, **k):
    TABLE.append(Entry(*a, **k))


def _c_rows_unit(c, M, N, batch):
    """plan_f32's c_rows_unit for a TT product of M x N: C's rows unit-stride for the SWAPPED product, everything on 16 B."""
    off, bs, ms, ns = C_LAYOUTS[c](M, N)
    return ns == 1 and ms % 4 == 0 and bs % 4 == 0 and off % 4 == 0 and N % 4 == 0


def _f32(id, lay, M, K, N, cfg, batch=1, a=PLAIN, b=PLAIN, c="contig", glds=1, nbuf=0, tt_swap=1, opts=None, note="", **kw):
    """A float32 product on the MFMA kernels with the tile forced; peel and repack off unless `opts` says otherwise."""
    o = {"gemm_cfg": cfg, "gemm_peel": 0, "gemm_repack": 0}
    if glds != 1:
        o["gemm_glds"] = glds
    if nbuf:
        o["gemm_nbuf"] = nbuf
    if tt_swap != 1:
        o["gemm_tt_swap"] = tt_swap
    o.update(opts or {})
    aligned = a.aligned and b.aligned
    if lay == "TT" and tt_swap:
        k, pool = _mfma_kernel(cfg, "NN", N, K, M, batch, glds, nbuf, aligned, ct=_c_rows_unit(c, M, N, batch), splitk=o.get("gemm_splitk", 1))
        k += " | TT swapped into NN"
    else:
        k, pool = _mfma_kernel(cfg, lay, M, K, N, batch, glds, nbuf, aligned, splitk=o.get("gemm_splitk", 1))
    _add(id, k + (" | " + note if note else ""), f32, M, K, N, batch, lay, a, b, c, o, (pool,), **kw)


LAYS = ("NN", "NT", "TN", "TT")

# ---- 1. register-staged k_gemm_f32_mfma: option gemm_glds = 0, every tile, the four layouts (TT as itself: gemm_tt_swap = 0) ------
for cfg in range(8):
    for li, lay in enumerate(LAYS):
        bm, bn, bk = REG[cfg][1 if lay == "TN" else 0][:3]
        _f32(f"reg-cfg{cfg}-{lay}-whole", lay, bm, 2 * bk, 2 * bn, cfg, glds=0, tt_swap=0, c=C_ALL[(cfg + li) % 6])
        kr = (0, 1, 4, 15)[(cfg + li) % 4]
        _f32(f"reg-cfg{cfg}-{lay}-edge-k{kr}", lay, bm + 1, 2 * bk + kr, 2 * bn - 1, cfg, glds=0, tt_swap=0, c=C_ALL[(cfg + li + 3) % 6])
for lay in LAYS:        # vec_ok = 0: operands off 16 B (a start one element in, an odd leading dimension)
    _f32(f"reg-cfg1-{lay}-misaligned", lay, 65, 36, 127, 1, a=Op(off=1), b=Op(pad=1), glds=0, tt_swap=0)
    _f32(f"reg-cfg3-{lay}-misaligned", lay, 257, 20, 129, 3, a=Op(pad=1), b=Op(off=1), glds=0, tt_swap=0, c="ms+1")
_f32("reg-cfg1-NN-batch3", "NN", 65, 33, 127, 1, batch=3, glds=0, c="bpad", a=Op(bpad=4))
_f32("reg-cfg1-TN-batch3", "TN", 64, 32, 128, 1, batch=3, glds=0, c="bpad2")
_f32("reg-cfg2-NT-batch3", "NT", 130, 20, 65, 2, batch=3, glds=0, c="T", b=Op(bpad=8))

# ---- 2. k_gemm_f32_kc_glds (NN, NT): 128 x 128 x 32 (cfg 0), eight waves (cfg 7), 256 x 256 x 32 (cfg 4) --------------------------
for cfg in (0, 7, 4):
    bm, bn, bk = DMA[cfg][0][:3]
    for lay in ("NN", "NT"):
        for nb in ((2, 3) if cfg != 4 else (2,)):      # (256 x 256 has no room for a third buffer)
            for kt in (1, 2, 3, 4, 5):                   # k-tiles: the pipeline prologues; at one k-tile the launcher keeps two buffers
                _f32(f"kc-cfg{cfg}-{lay}-nbuf{nb}-kt{kt}", lay, bm, kt * bk, 2 * bn, cfg, nbuf=nb, c=C_ALL[(kt + nb) % 6])
    # RAGGED = 2 (128-row tiles) / 1 (256): ragged M or N under whole k-tiles
    _f32(f"kc-cfg{cfg}-NN-ragged-mn", "NN", bm + 1, 2 * bk, 2 * bn - 4, cfg, c="ms+4")
    _f32(f"kc-cfg{cfg}-NT-ragged-mn", "NT", bm - 1, 2 * bk, bn + 1, cfg, c="ms+1", a=Op(pad=4), b=Op(pad=8))
    # RAGGED = 1: K % 32 in {4, 16, 28}
    for kr in (4, 16, 28):
        _f32(f"kc-cfg{cfg}-NN-ragged-k{kr}", "NN", bm, 2 * bk + kr, bn + (0 if kr == 16 else 4), cfg, c="off1" if kr == 4 else "contig")
    _f32(f"kc-cfg{cfg}-NT-ragged-k28", "NT", bm + 3, bk + 28, bn - 3, cfg, c="T")
    # NN with N % 4 != 0: not whole 16-B pieces -> the register-staged edge kernel
    _f32(f"kc-cfg{cfg}-NN-n-odd", "NN", bm, 2 * bk, 2 * bn - 2, cfg, note="N % 4 != 0 falls to the register-staged kernel")
    _f32(f"kc-cfg{cfg}-NN-padded-rows", "NN", bm, 3 * bk, bn, cfg, a=Op(pad=4, off=4), b=Op(pad=8), batch=2, c="bpad")
# CT: the TT product swapped into NN, c_vec_rows on for exactly the C layouts that allow it — every C layout
for c in C_ALL + ("Toff1", "bpad2"):
    _f32(f"kc-cfg0-TT-swap-{c}", "TT", 256, 64, 128, 0, c=c, batch=2 if c.startswith("bpad") else 1)
    _f32(f"kc-cfg7-TT-swap-ragged-{c}", "TT", 132, 40, 126, 7, c=c, batch=2 if c.startswith("bpad") else 1)
_f32("kc-cfg4-TT-swap", "TT", 256, 96, 512, 4)
_f32("reg-cfg1-TT-swap", "TT", 128, 48, 64, 1, note="swapped, register-staged")
_f32("kc-cfg0-TT-noswap", "TT", 256, 64, 128, 0, tt_swap=0)

# ---- 3. k_gemm_f32_tn_glds: 256 x 256 x 32 (cfg 4), 128 x 128 x 32 (cfg 5), 128 x 64 x 32 (cfg 6), eight waves (cfg 7) -------------
for cfg in (4, 5, 6, 7):
    bm, bn, bk = DMA[cfg][1][:3]
    for nb in ((2, 3) if cfg != 4 else (2,)):
        for kt in (1, 2, 3, 4, 5):
            _f32(f"tn-cfg{cfg}-nbuf{nb}-kt{kt}", "TN", bm, kt * bk, 2 * bn, cfg, nbuf=nb, c=C_ALL[(kt + nb + 1) % 6])
    _f32(f"tn-cfg{cfg}-ragged-mn", "TN", bm + 4, 2 * bk, 2 * bn - 4, cfg, c="ms+4")
    for kr in (4, 16, 28):
        _f32(f"tn-cfg{cfg}-ragged-k{kr}", "TN", bm + (4 if kr == 4 else 0), bk + kr, bn, cfg, c="T" if kr == 28 else "contig")
    _f32(f"tn-cfg{cfg}-m-odd", "TN", bm + 2, 2 * bk, bn, cfg, note="M % 4 != 0: dma_pieces_whole refuses")
    _f32(f"tn-cfg{cfg}-padded-rows", "TN", bm, 2 * bk, bn, cfg, a=Op(pad=8), b=Op(pad=4, off=8), batch=2, c="bpad")

# ---- 4. tile numbering: super_h bands (option gemm_super) and the XCD remap, register-staged and direct-to-LDS -----------------
_f32("super2-reg-320x512", "NN", 320, 64, 512, 1, glds=0, opts={"gemm_super": 2}, note="bands of 2, 2, 1 tile rows")
_f32("super2-tn-640x512", "TN", 640, 64, 512, 6, opts={"gemm_super": 2}, note="bands of 2, 2, 1 tile rows")
_f32("super2-kc-640x1024", "NN", 640, 64, 1024, 0, opts={"gemm_super": 2}, note="bands of 2, 2, 1 tile rows", c="ms+4")
for tm in (8, 9, 15):   # the default band height 8: one whole band; a short second band of 1 and of 7
    _f32(f"super8-reg-tm{tm}", "NN", 64 * tm, 32, 512, 1, glds=0, note=f"tiles_m {tm}, super_h 8")
    _f32(f"super8-tn-tm{tm}", "TN", 128 * tm, 32, 512, 6, note=f"tiles_m {tm}, super_h 8")
    _f32(f"super8-kc-tm{tm}", "NT", 128 * tm, 32, 1024, 7, note=f"tiles_m {tm}, super_h 8")
_f32("super0-reg-576x512", "NN", 576, 32, 512, 1, glds=0, opts={"gemm_super": 0}, note="plain row-major numbering")

# ---- 5. in-kernel split-K + k_gemm_splitk_sum (the cost model's early return picks 64 x 64: gemm_cfg stays -1) -----------------
for K in (1024, 1040, 1030, 2048 + 16):     # even splits | a short last chunk | a last chunk that is no multiple of 16 | the cap K / 512
    for (M, N, batch, lay, c) in ((64, 64, 1, "NN", "ms+4"), (64, 128, 2, "NN", "T"), (64, 128, 2, "TN", "contig"), (64, 64, 1, "NT", "off1")):
        if lay in ("TN", "NT") and K not in (1030, 2064):
            continue
        for sk in (1, 0):
            k, pool = _mfma_kernel(1, lay, M, K, N, batch, splitk=sk)
            _add(f"splitk{'' if sk else '-off'}-{lay}-{M}x{K}x{N}", k, f32, M, K, N, batch, lay, c=c if sk else "contig", pool=(pool,),
                 opts={"gemm_peel": 0, "gemm_splitk": sk}, rep=bool(sk))

# ---- 6. k ranges (plan_kranges): integer data only (float64 matmul reference), milliseconds on the device -------------------------
def _kranges(M, K, N):
    t128, t64 = -(-M // 128) * -(-N // 128), -(-M // 64) * -(-N // 64)
    assert t64 >= CUS and t128 <= CUS // 2 and max(M, N) <= 2048 and K >= 4096 and K >= 2 * max(M, N)
    splits = min(CUS // t128, 4)
    chunk = K // splits // 32 * 32
    assert splits >= 2 and chunk >= 1024
    return splits, chunk, K - splits * chunk


for (M, K, N, c) in ((1024, 4096, 1024, "contig"), (1024, 4096 + 40, 1024, "ms+4"), (1408, 4096, 768, "contig")):
    splits, chunk, rem = _kranges(M, K, N)
    _add(f"kranges-{M}x{K}x{N}", f"k ranges: a batch of {splits} products of k {chunk}" + (f", a remainder product of k {rem}" if rem else "") +
         " (tiles by the cost model) + k_gemm_splitk_sum", f32, M, K, N, c=c, pool=((splits + (rem > 0)) * M * N * 4,), flt=False, rep=(rem > 0))

# ---- 7. repack (k_repack_rows): misaligned operands of a large product copied into aligned buffers, then the DMA kernels ----------
ODD = Op(pad=1, off=1)
for lay, cfg in (("NN", 0), ("NT", 0), ("TN", 5)):
    for (M, K, N) in ((256, 256, 256), (260, 256, 257)):
        for who in ("a", "b", "ab"):
            a_op, b_op = (ODD if "a" in who else PLAIN), (ODD if "b" in who else PLAIN)
            a_kc, b_kc = lay in ("NN", "NT"), lay == "NT"
            pool = []
            if "a" in who:
                pool.append((M * _ceil4(K) if a_kc else K * _ceil4(M)) * 4)
            if "b" in who:
                pool.append((N * _ceil4(K) if b_kc else K * _ceil4(N)) * 4)
            k, _ = _mfma_kernel(cfg, lay, M, K, N, pad_m="a" in who and not a_kc, pad_n="b" in who and not b_kc)
            _add(f"repack-{lay}-{who}-{M}x{K}x{N}", "k_repack_rows + " + k, f32, M, K, N, lay=lay, a=a_op, b=b_op, c="ms+1" if who == "ab" else "contig",
                 pool=pool, opts={"gemm_cfg": cfg, "gemm_peel": 0})
_f32("repack-off-NN-256", "NN", 256, 256, 256, 0, a=ODD, note="gemm_repack = 0: the register-staged edge kernel")

# ---- 8. peel (option gemm_peel = 2): main block + bottom strip + right strip, with the skinny hand-off in front of a strip ---------
def _peel(id, lay, M, K, N, cfg, c="contig", **kw):
    Mm, Nm = M // 256 * 256, N // 256 * 256
    if lay == "TT":
        (M, N), lay2 = (N, M), "NN"
        Mm, Nm = M // 256 * 256, N // 256 * 256
    else:
        lay2 = lay
    parts, pool = [], []
    if K % 32 or not Mm or not Nm or (M == Mm and N == Nm):
        parts.append(_mfma_kernel(cfg, lay2, M, K, N)[0] + " | peel refused")
    else:
        ct = lay == "TT" and _c_rows_unit(c, N, M, 1)
        parts.append(_mfma_kernel(cfg, lay2, Mm, K, Nm, ct=ct)[0])
        for (m, n) in ((M - Mm, N), (Mm, N - Nm)):
            if m and n:
                sk = _skinny(f32, lay2, m, K, n, 1)
                parts.append(sk[0] if sk else _mfma_kernel(cfg, lay2, m, K, n)[0])
                pool.append(sk[1] if sk else 0)
    _add(id, " + ".join(parts), f32, kw.pop("M0", M), K, kw.pop("N0", N), lay=lay, c=c, pool=pool, opts={"gemm_cfg": cfg, "gemm_peel": 2}, rep=True, **kw)


def _skinny(dt, lay, M, K, N, batch, aligned=True, a_ld=None, b_ld=None):
    """md_gemm_skinny restated for PLAIN operands -> (kernel name, pool bytes) or None (declined)."""
    V = 16 // dt.itemsize
    T = "float" if dt == f32 else "double"
    if N <= 8 < M:
        R, nc, x_kc = M, N, lay in ("NN", "NT")
    elif M <= 8 < N:
        R, nc, x_kc = N, M, lay in ("NT", "TT")
    else:
        return None
    if R < 512 or K < 64 or R * K * batch < (1 << 20) or not aligned:
        return None
    nct = 1 if nc == 1 else 2 if nc == 2 else 4 if nc <= 4 else 8
    if x_kc:
        if K % V:
            return None
        return f"k_skinny_rowdot<{T}, {nct}, {4 if R >= 8192 else 2 if R >= 4096 else 1}>", 0
    if R % V:
        return None
    NS = -(-R // (64 * V))
    NB = max(1, min(-(-1024 // (NS * batch)), 64, K // 32))
    if NB > 1 and NS * batch * 16 > 16384:
        NB = 1
    return f"k_skinny_colsum<{T}, {nct}, 8>" + (f" | NB {NB}" if NB > 1 else " | NB 1"), (batch * NB * nct * R * dt.itemsize if NB > 1 else 0)


for r in (1, 9, 130):
    _peel(f"peel-NN-bottom{r}", "NN", 256 + r, 64, 256, 0)
    _peel(f"peel-NN-right{r}", "NN", 256, 64, 256 + r, 0)
    _peel(f"peel-TN-both{r}", "TN", 256 + r, 64, 256 + r, 5, c="ms+4")
_peel("peel-TN-both132", "TN", 388, 64, 388, 5, c="T")                            # strips on the ragged direct-to-LDS kernel
_peel("peel-NN-bottom8-skinny", "NN", 256 + 8, 1024, 1024, 0, c="ms+4")          # strip 8 x 1024 x 1024: colsum takes it
_peel("peel-NN-right8-skinny", "NN", 512, 2048, 256 + 8, 0)                      # strip 512 x 2048 x 8: rowdot takes it
_peel("peel-NN-k48-refused", "NN", 260, 48, 256, 0)
_peel("peel-TT-swap", "TT", 264, 64, 260, 0, M0=264, N0=260)

# ---- 9. skinny.hip -------------------------------------------------------------------------------------------------------------------
def _thin(id, dt, lay, M, K, N, batch=1, c="contig", a=PLAIN, b=PLAIN, opts=None, **kw):
    o = {"gemm_peel": 0, "gemm_repack": 0}
    o.update(opts or {})
    sk = _skinny(dt, lay, M, K, N, batch, a.aligned and b.aligned) if o.get("gemm_skinny", 1) else None
    if sk:
        _add(id, sk[0], dt, M, K, N, batch, lay, a, b, c, o, (sk[1],), rep=True, **kw)
    else:
        _add(id, "declined by md_gemm_skinny: the MFMA / generic kernels", dt, M, K, N, batch, lay, a, b, c, o, **kw)


for (R, K) in ((1024, 1024), (4096, 256), (8192, 128)):       # RW 1 / 2 / 4 at the smallest K with R K >= 2^20
    for nc in (1, 2, 3, 5, 8):                                  # NCT 1 / 2 / 4 / 8
        _thin(f"rowdot-f32-R{R}-nc{nc}", f32, "NN", R, K, nc, c=("contig", "T", "Toff1", "ms+1", "ms+4")[nc % 5], public=(nc == 3))
for (R, K, nc, c) in ((1024, 1024, 2, "T"), (4096, 256, 5, "contig"), (8192, 128, 1, "Toff1")):
    _thin(f"rowdot-f64-R{R}-nc{nc}", f64, "NN", R, K, nc, c=c)
_thin("rowdot-f32-thin-m", f32, "NT", 3, 1024, 1024, c="ms+4")
_thin("rowdot-f64-thin-m", f64, "NT", 8, 512, 2048, c="T")
_thin("rowdot-f32-batch", f32, "NN", 512, 512, 4, batch=4, c="bpad")
for nc, c in ((1, "T"), (2, "Toff1"), (4, "contig"), (7, "ms+4")):          # X r-contiguous: the weighted column sum, NB > 1
    _thin(f"colsum-f32-nc{nc}", f32, "TN", 1024, 1024, nc, c=c, public=(nc == 4))
    _thin(f"colsum-f64-nc{nc}", f64, "TN", 1024, 1024, nc, c=c)
_thin("colsum-f32-thin-m", f32, "NN", 5, 1024, 1028, c="contig")          # o_r = c_ns = 1: the vector store
_thin("colsum-f32-thin-m-off1", f32, "NN", 5, 1024, 1028, c="off1")       # .. misaligned: scalar stores
_thin("colsum-f64-thin-m", f64, "TN", 2, 2048, 512, c="ms+1")
_thin("colsum-f32-nb1", f32, "TN", 512, 64, 2, batch=513, c="contig")     # NS batch 16 > 16384: no tickets, NB = 1
# every decline falls through and is still exact
_thin("skinny-decline-R256", f32, "NN", 256, 4096, 3)
_thin("skinny-decline-K-odd", f32, "NN", 1024, 1022, 3, a=Op())            # K % V != 0 (rowdot) and X not r-contiguous
_thin("skinny-decline-misaligned", f32, "NN", 1024, 1024, 3, a=Op(off=1))
_thin("skinny-decline-f64-K-odd", f64, "NN", 1024, 1023, 2)
_thin("skinny-off", f32, "NN", 1024, 1024, 3, opts={"gemm_skinny": 0})

# ---- 10. long-k (k_longk_partial + k_longk_finish) ------------------------------------------------------------------------------
CT_NAME = {f32: "float", f64: "double", i32: "int", i64: "long"}


def _longk(id, dt, M, K, N, batch=1, c="contig", lay="NN", **kw):
    big, small = max(M, N), min(M, N)
    takes = M <= 128 and N <= 128 and (K >= 512 if big <= 8 else (K >= 8192 and K >= 64 * big and not (dt == f32 and small >= 64)))
    if not takes:
        if dt == f32 and M * N >= 4096 and K >= 1024:
            k, pool = _mfma_kernel(1, lay, M, K, N, batch)
            return _add(id, k + " | long-k declines float32 from 64 x 64 up", dt, M, K, N, batch, lay, c=c, pool=(pool,), opts={"gemm_peel": 0}, rep=True, **kw)
        return _add(id, "declined by md_gemm_longk", dt, M, K, N, batch, lay, c=c, opts={"gemm_peel": 0}, **kw)
    tm, tn = ((1, 1) if (M, N) == (1, 1) else (2, 2) if big <= 2 else (4, 4) if big <= 4 else (8, 1) if N == 1 else (1, 8) if M == 1 else (8, 8))
    patches = batch * -(-M // tm) * -(-N // tn)
    nb = min(-(-K // 4096), 1 if patches >= 1024 else 1024 // patches)
    nb = -(-K // -(-K // nb))
    _add(id, f"k_longk_partial<{CT_NAME[dt]}, {tm}, {tn}> + k_longk_finish<{CT_NAME[dt]}, {tm}, {tn}>", dt, M, K, N, batch, lay, c=c,
         pool=(patches * nb * tm * tn * dt.itemsize,), rep=True, **kw)


for (M, N) in ((1, 1), (2, 2), (4, 4), (8, 1), (1, 8), (8, 8), (3, 3), (5, 7)):
    for K in (512, 4097, 70000):
        for dt in (f32, f64, i32, i64):
            _longk(f"longk-{dt.name}-{M}x{K}x{N}", dt, M, K, N, c=("contig", "ms+4", "T")[(M + K) % 3], lay=LAYS[(M + N + K) % 4],
                   public=(dt == i64 and K == 4097 and M == 5))
for dt in (f32, f64, i32, i64):
    _longk(f"longk-{dt.name}-9x70000x1", dt, 9, 70000, 1, c="ms+1")                      # two 8 x 1 patches, the second one row high
    _longk(f"longk-{dt.name}-16x8192x16", dt, 16, 8192, 16, c="ms+4")                    # K >= 8192 and K >= 64 max(M, N)
    _longk(f"longk-{dt.name}-64x8192x64", dt, 64, 8192, 64)                              # float32: excluded (split-K MFMA)
    _longk(f"longk-{dt.name}-batch3", dt, 2, 4097, 2, batch=3, c="bpad")
_longk("longk-f32-16x8191x16-declined", f32, 16, 8191, 16)

# ---- 11. k_gemm_generic ----------------------------------------------------------------------------------------------------------
for dt in (f32, f64, i32, i64):
    g = f"k_gemm_generic<{CT_NAME[dt]}>"
    o = {"gemm_peel": 0, "gemm_repack": 0}
    _add(f"generic-{dt.name}-small", g + " | M N < 4096", dt, 33, 29, 17, lay="NN", c="ms+1", opts=o, public=(dt == i32))
    _add(f"generic-{dt.name}-k5", g + " | K < 8", dt, 100, 5, 100, lay="TN", c="T", opts=o)
    _add(f"generic-{dt.name}-step2", g + " | both strides of A non-unit", dt, 80, 40, 80, lay="NN", a=Op(kind="step2"), opts=o)
    _add(f"generic-{dt.name}-step2-b", g + " | both strides of B non-unit", dt, 80, 40, 80, lay="NT", b=Op(kind="step2"), batch=2, c="bpad", opts=o)
    _add(f"generic-{dt.name}-flip", g + " | negative stride", dt, 70, 33, 90, lay="NN", a=Op(kind="flip"), b=Op(kind="flip"), opts=o)
    _add(f"generic-{dt.name}-bcast", g + " | stride 0 across the rows of A", dt, 40, 33, 50, lay="NN", a=Op(kind="bcast"), opts=o)
    if dt.kind == "i":
        _add(f"generic-{dt.name}-large", g + " | integers have no other kernel", dt, 130, 70, 129, lay="TT", batch=2, c="ms+4", opts=o)
_add("generic-f64-mfma-off", "k_gemm_generic<double> | gemm_f64_mfma = 0", f64, 128, 32, 128, opts={"gemm_f64_mfma": 0})
_add("reg-cfg1-NN-bcast-rows", _reg(T64, True, False, False) + " | a_ms = 0", f32, 64, 32, 128, a=Op(kind="bcast"),
     opts={"gemm_cfg": 1, "gemm_peel": 0, "gemm_repack": 0, "gemm_glds": 0})

# ---- 12. float64 -------------------------------------------------------------------------------------------------------------------
def _f64k(bm, lay, edge):
    return f"k_gemm_f64_mfma<{bm}, {bm}, 16, 2, 2, {_b(lay in ('NN', 'NT'))}, {_b(lay in ('NT', 'TT'))}, {_b(edge)}>"


for li, lay in enumerate(LAYS):
    _add(f"f64-64-{lay}-whole", _f64k(64, lay, False), f64, 128, 32, 64, lay=lay, c=C_ALL[li], public=(lay == "NT"))
    _add(f"f64-64-{lay}-edge", _f64k(64, lay, True), f64, 65, 16 + (0, 1, 4, 15)[li], 127, lay=lay, c=C_ALL[li + 2], batch=2 if lay == "NT" else 1)
    _add(f"f64-64-{lay}-misaligned", _f64k(64, lay, True), f64, 64, 32, 128, lay=lay, a=Op(off=1), b=Op(pad=1))
# 128 x 128: batch x t128 >= 512
_add("f64-128-NN-whole", _f64k(128, "NN", False), f64, 1024, 16, 1024, batch=8)
_add("f64-128-TN-whole-k16", _f64k(128, "TN", False) + " | K = 16: the direct-to-LDS kernel refuses", f64, 1024, 16, 1024, batch=8, lay="TN", c="bpad")
_add("f64-128-NT-edge", _f64k(128, "NT", True), f64, 1020, 17, 1028, batch=8, lay="NT")
_add("f64-128-TT-edge", _f64k(128, "TT", True), f64, 1025, 16, 1024, batch=8, lay="TT", c="ms+1", flt=False)
_add("f64-tn-glds-2048", "k_gemm_f64_tn_glds", f64, 2048, 32, 2048, lay="TN", c="ms+4")
_add("f64-tn-glds-batch4", "k_gemm_f64_tn_glds", f64, 1024, 48, 1024, batch=4, lay="TN", c="bpad", a=Op(pad=2))
_add("f64-tn-glds-m-ragged", _f64k(64, "TN", False) + " | M % 128 != 0: refused", f64, 2048 + 64, 32, 2048, lay="TN", flt=False)
_add("f64-tn-glds-off", _f64k(64, "TN", False) + " | gemm_glds = 0", f64, 2048, 32, 2048, lay="TN", opts={"gemm_glds": 0}, flt=False)

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE), [e.id for e in TABLE if sum(x.id == e.id for x in TABLE) > 1]
assert all(9 * e.K < 2 ** 24 for e in TABLE)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("MDHIP_MATMUL_PATHS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float products of tests/test_matmul_paths.py: largest |got - ref| / (1.01 K u (|a| @ |b|)) per path (bound: 1)\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key]:8.5f}  {key}\n")


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


def _rng(e, salt):
    return np.random.default_rng([TABLE.index(e), salt])


def _filler(dt, n, rng):
    if dt.kind == "f":
        return np.full(n, np.nan, dtype=dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def _place(x, trans, op, rng):
    """The logical (B, R, C) operand inside its base: -> (flat base, offset, element strides of the logical axes)."""
    st = x.transpose(0, 2, 1) if trans else x
    B, rows, cols = st.shape
    cs = 2 if op.kind == "step2" else -1 if op.kind == "flip" else 1
    ld = _ceil4(cols * abs(cs)) + op.pad
    rs = 0 if op.kind == "bcast" else ld
    bs = (1 if op.kind == "bcast" else rows) * ld + op.bpad
    off = op.off + (cols - 1 if cs < 0 else 0)
    flat = _filler(x.dtype, op.off + B * bs + 8, rng)
    idx = off + np.arange(B)[:, None, None] * bs + np.arange(rows)[None, :, None] * rs + np.arange(cols)[None, None, :] * cs
    flat[idx] = st
    return flat, off, ((bs, cs, rs) if trans else (bs, rs, cs))


def _operands(e, A, B, rng):
    """Device views of A (batch, M, K) and B (batch, K, N) in the entry's layout (the bases stay alive with the views)."""
    out = []
    for x, trans, op in ((A, e.lay in ("TN", "TT"), e.a), (B, e.lay in ("NT", "TT"), e.b)):
        flat, off, strides = _place(x, trans, op, rng)
        out.append(nd.asarray(flat)._view(off, x.shape, strides))
    return out


def _bcast_rows(e, A, B):
    """stride 0 across the stored rows: the logical operand repeats its first stored row."""
    if e.a.kind == "bcast":
        A = np.ascontiguousarray(np.broadcast_to(A[:, :, :1] if e.lay in ("TN", "TT") else A[:, :1, :], A.shape))
    if e.b.kind == "bcast":
        B = np.ascontiguousarray(np.broadcast_to(B[:, :1, :] if e.lay in ("NT", "TT") else B[:, :, :1], B.shape))
    return A, B


def _poison_pool(e):
    """Blocks of the byte sizes the plan's temporaries take, full of NaN (float64 entries: float64 NaN), back on the free lists."""
    fill = e.dt if e.dt.kind == "f" else f32
    blocks = [nd.asarray(np.full(n // fill.itemsize, np.nan, dtype=fill)) for n in e.pool]     # (all live at once: distinct blocks)
    del blocks


SENTINEL = 0xA5


def _run(e, A, B, rng, via_public=False):
    """C = A @ B of the entry through the C-ABI into a sentinel-filled base -> the view's values (surroundings checked)."""
    da, db = _operands(e, A, B, rng)
    if via_public:
        if TABLE.index(e) % 2 == 0 or e.dt.kind == "i":
            out = nd.asarray(np.full((e.batch, e.M, e.N), SENTINEL, dtype=np.uint8).astype(e.dt))
            r = nd.matmul(da, db, out=out)
            assert r is out
            return out.get()
        return nd.matmul(da, db).get()
    off, bs, ms, ns = C_LAYOUTS[e.c](e.M, e.N)
    n = off + e.batch * bs + 8
    base = nd.asarray(np.full(n * e.dt.itemsize, SENTINEL, dtype=np.uint8).view(e.dt))
    dc = base._view(off, (e.batch, e.M, e.N), (bs, ms, ns))
    _poison_pool(e)
    nd._lib().matmul(da.desc(), db.desc(), dc.desc())
    flat = base.get()
    idx = off + np.arange(e.batch)[:, None, None] * bs + np.arange(e.M)[None, :, None] * ms + np.arange(e.N)[None, None, :] * ns
    outside = np.ones(n, dtype=bool)
    outside[idx] = False
    assert (flat.view(np.uint8).reshape(n, -1)[outside] == SENTINEL).all(), (e.id, "bytes of C's base outside the view were written")
    return flat[idx]


def _exact_data(e, rng):
    shape_a, shape_b = (e.batch, e.M, e.K), (e.batch, e.K, e.N)
    if e.dt.kind == "f":
        A, B = rng.choice(np.array([-3, -1, 1, 3], dtype=e.dt), shape_a), rng.choice(np.array([-3, -1, 1, 3], dtype=e.dt), shape_b)
        A, B = _bcast_rows(e, A, B)
        ref = np.matmul(A.astype(f64), B.astype(f64))       # exact: odd integers, |sum| <= 9 K < 2^24
        assert np.abs(ref).max() < 2 ** 24 and (ref % 2 == e.K % 2).all()
        return A, B, ref.astype(e.dt)
    info = np.iinfo(e.dt)
    A, B = (rng.integers(info.min, info.max, s, dtype=e.dt, endpoint=True) for s in (shape_a, shape_b))
    A, B = _bcast_rows(e, A, B)
    return A, B, np.matmul(A, B)                            # NumPy's wrap-around in the same dtype


def _float_data(e, rng):
    A, B = rng.standard_normal((e.batch, e.M, e.K)).astype(e.dt), rng.standard_normal((e.batch, e.K, e.N)).astype(e.dt)
    return _bcast_rows(e, A, B)


# md_options.h defaults of everything an entry may set: put back before every entry (the interleaved tests run many in one test)
DEFAULTS = {"gemm_cfg": -1, "gemm_glds": 1, "gemm_nbuf": 0, "gemm_peel": 1, "gemm_tt_swap": 1, "gemm_repack": 1, "gemm_super": 8, "gemm_splitk": 1,
            "gemm_f64_mfma": 1, "gemm_skinny": 1}


def _set_opts(e, mdopt, extra=None):
    for k, v in {**DEFAULTS, **e.opts, **(extra or {})}.items():
        mdopt(k, v)


def _float_check(e, A, B, got, extra=""):
    wide = np.longdouble if e.dt == f64 else np.float64
    rows = np.arange(e.M)
    if e.dt == f64 and e.work > (1 << 24):                  # (longdouble has no BLAS: a spread of 16 rows of every batch)
        rows = np.unique(np.linspace(0, e.M - 1, 16).astype(np.int64))
    a = A[:, rows].astype(wide)
    ref, mass = np.matmul(a, B.astype(wide)), np.matmul(np.abs(a), np.abs(B).astype(wide))
    u = wide(2.0) ** (-24 if e.dt == f32 else -53)
    bound = wide(1.01) * e.K * u * mass
    err = np.abs(got[:, rows].astype(wide) - ref)
    ratio = float((err / bound).max())
    key = e.reaches + extra
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    assert np.isfinite(got).all() and ratio <= 1.0, (e.id, ratio)


def _check_entry(e, mdopt, on_gpu, via_public=False):
    if not on_gpu and not e.cpu:
        pytest.skip("batch M N K > 2^24: the CPU double is a triple loop")
    _set_opts(e, mdopt)
    A, B, ref = _exact_data(e, _rng(e, 1))
    got = _run(e, A, B, _rng(e, 2), via_public)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref, err_msg=f"{e.id}: {e.reaches}")
    if e.flt:
        A, B = _float_data(e, _rng(e, 3))
        _float_check(e, A, B, _run(e, A, B, _rng(e, 4), via_public), " public" if via_public else "")


IDS = [e.id for e in TABLE]


@_twins(IDS)
def _kernel_paths(case, mdopt, on_gpu):
    _check_entry(BY_ID[case], mdopt, on_gpu)


test_kernel_paths, test_kernel_paths_gpu = _kernel_paths

PUBLIC = [e.id for e in TABLE if e.public] + ["reg-cfg1-NN-batch3", "kc-cfg0-NN-nbuf3-kt3", "tn-cfg5-ragged-mn", "splitk-NN-64x1030x64",
                                              "repack-TN-ab-260x256x257", "peel-TN-both9", "kc-cfg0-TT-swap-contig"]


@_twins(PUBLIC)
def _public_functions(case, mdopt, on_gpu):
    """A subset through nd.matmul on the same operand views (a fresh C-contiguous result, or `out=` pre-filled with a wrong value)."""
    _check_entry(BY_ID[case], mdopt, on_gpu, via_public=True)


test_public_functions, test_public_functions_gpu = _public_functions


def test_table_covers_the_size_rule():
    """Every entry is either small enough for the CPU double or says what it reaches only at that size; the CPU half is not empty
    for any section."""
    sections = {}
    for e in TABLE:
        sections.setdefault(e.id.split("-")[0], []).append(e.cpu)
    assert all(any(v) for k, v in sections.items() if k not in ("kranges",)), {k: any(v) for k, v in sections.items()}


# ---- bit-identity groups ---------------------------------------------------------------------------------------------------------
# (id, layout, M, K, N, batch, a, b, fixed options, members): every member's result equals the first member's bit for bit.
# Which forms share a summation order (gemm.hip): the register-staged kernel and the TN direct-to-LDS kernel feed
# v_mfma_f32_32x32x2 the k pairs (0, 1), (2, 3), ..; the NN / NT direct-to-LDS kernel feeds it (0, 4), (1, 5), .. of every eight
# (its k-contiguous LDS image) — "a different rounding sequence from the register-staged kernel", so NN / NT under gemm_glds = 1
# form a group of their own (the DMA tiles), apart from the register-staged tiles.
OFF = {"gemm_peel": 0, "gemm_repack": 0}
GROUPS = [
    ("cfg-all-eight-reg-" + lay, lay, 256, 80, 256, 1, PLAIN, PLAIN, {**OFF, "gemm_glds": 0, "gemm_tt_swap": 0}, [{"gemm_cfg": c} for c in range(8)])
    for lay in LAYS
] + [
    ("cfg-all-eight-TN-dma", "TN", 256, 96, 256, 1, PLAIN, PLAIN, OFF, [{"gemm_cfg": c} for c in range(8)]),
    ("cfg-dma-tiles-NN", "NN", 256, 96, 256, 1, PLAIN, PLAIN, OFF, [{"gemm_cfg": c} for c in (0, 4, 5, 7)]),
    ("cfg-dma-tiles-NT", "NT", 256, 96, 256, 1, PLAIN, PLAIN, OFF, [{"gemm_cfg": c} for c in (0, 4, 5, 7)]),
    ("cfg-reg-tiles-NN-glds-on", "NN", 256, 96, 256, 1, PLAIN, PLAIN, OFF, [{"gemm_cfg": c} for c in (1, 2, 3, 6)]),
    ("glds-TN", "TN", 256, 160, 256, 2, PLAIN, PLAIN, {**OFF, "gemm_cfg": 5}, [{"gemm_glds": 1}, {"gemm_glds": 0}]),
    ("glds-TN-ragged", "TN", 260, 100, 252, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 7}, [{"gemm_glds": 1}, {"gemm_glds": 0}]),
    ("nbuf-NN", "NN", 128, 160, 256, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 0}, [{"gemm_nbuf": 2}, {"gemm_nbuf": 3}, {"gemm_nbuf": 0}]),
    ("nbuf-NT-w8", "NT", 128, 128, 256, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 7}, [{"gemm_nbuf": 2}, {"gemm_nbuf": 3}]),
    ("nbuf-TN", "TN", 128, 160, 128, 2, PLAIN, PLAIN, {**OFF, "gemm_cfg": 6}, [{"gemm_nbuf": 2}, {"gemm_nbuf": 3}]),
    ("super-reg", "NN", 320, 64, 512, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 1, "gemm_glds": 0}, [{"gemm_super": 0}, {"gemm_super": 2}, {"gemm_super": 8}]),
    ("super-tn", "TN", 1152, 64, 512, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 6}, [{"gemm_super": 0}, {"gemm_super": 2}, {"gemm_super": 8}]),
    ("tt-swap-reg", "TT", 128, 80, 256, 1, PLAIN, PLAIN, {**OFF, "gemm_cfg": 0, "gemm_glds": 0}, [{"gemm_tt_swap": 1}, {"gemm_tt_swap": 0}]),
    ("repack-TN", "TN", 260, 256, 257, 1, ODD, ODD, {"gemm_peel": 0, "gemm_cfg": 5}, [{"gemm_repack": 1}, {"gemm_repack": 0}]),
    ("repack-NN-reg", "NN", 256, 256, 260, 1, ODD, PLAIN, {"gemm_peel": 0, "gemm_cfg": 0, "gemm_glds": 0}, [{"gemm_repack": 1}, {"gemm_repack": 0}]),
]


@_twins([g[0] for g in GROUPS])
def _bit_identity(case, mdopt, on_gpu):
    id_, lay, M, K, N, batch, a, b, fixed, members = next(g for g in GROUPS if g[0] == case)
    e = Entry(id_, "group", f32, M, K, N, batch, lay, a, b, "ms+4", fixed)
    if not on_gpu and e.work * len(members) > 4 * CPU_MAX:
        pytest.skip("too large for the CPU double's triple loop")
    rng = np.random.default_rng([len(TABLE), GROUPS.index(next(g for g in GROUPS if g[0] == case))])
    A, B = _float_data(e, rng)
    first = None
    for m in members:
        _set_opts(e, mdopt, m)
        got = _run(e, A, B, np.random.default_rng(5))
        if first is None:
            first = got
            _float_check(e, A, B, got)
        else:
            diff = int((got.view(np.uint32) != first.view(np.uint32)).sum())
            assert diff == 0, (case, m, f"{diff} of {got.size} outputs differ from {members[0]}")


test_bit_identity, test_bit_identity_gpu = _bit_identity

# ---- the order-changing forms repeat their bits ---------------------------------------------------------------------------------
REPEATED = [e.id for e in TABLE if e.rep and e.dt.kind == "f"]


@_twins(["repeats"])
def _repeats_give_the_same_bits(case, mdopt, on_gpu):
    """Split-K, k ranges, peeled strips, skinny (partial planes + tickets) and long-k (block partials) three times, interleaved
    with each other, the pool poisoned before every call: each repeat must give the bits of the first. A ticket counter left off
    zero, or a partial plane read from another launch, makes a later launch that shares the word merge early or never."""
    # (the double has no tickets and no pool, and is a triple loop: a third of its CPU-sized entries proves the plumbing)
    ids = REPEATED if on_gpu else [i for i in REPEATED if BY_ID[i].cpu][::3]
    assert len(ids) >= 10
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
            got = _run(e, A, B, _rng(e, 7)).tobytes()
            assert first.setdefault(k, got) == got, (e.id, e.reaches)


test_repeats_give_the_same_bits, test_repeats_give_the_same_bits_gpu = _repeats_give_the_same_bits


# ---- 13. the fused epilogue mdhip_matmul_bias_relu_sum, called directly ---------------------------------------------------------
# (id, reaches, M, K, N, options, padded a rows). plan_epi: the DMA form for whole 32-deep k-tiles when the forced tile's
# direct-to-LDS form divides the problem; else the register-staged tile of the choice, then 128x128 after 256x128, 128x64, 64x64 —
# the register form only where the PLAIN product is register-staged too (tiles 1, 2, 3, 6, or gemm_glds = 0): see EPI_REFUSALS.
def _epi_reg(t):
    return f"k_gemm_f32_mfma<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, true, false, false, false, {0 if t[0] == 64 else 1}, 1>"


EPI = [
    ("epi-dma-128", _kc(D128, False, epi=1), 128, 64, 256, {"gemm_cfg": 0}, 0),
    ("epi-dma-w8", _kc(W8, False, epi=1), 256, 96, 128, {"gemm_cfg": 7}, 4),
    ("epi-dma-256", _kc(D256, False, epi=1), 256, 64, 512, {"gemm_cfg": 4}, 0),
    ("epi-reg-k48", _epi_reg(T128x64), 128, 48, 256, {"gemm_cfg": 2}, 0),
    ("epi-reg-glds-off", _epi_reg(T128), 128, 64, 128, {"gemm_cfg": 0, "gemm_glds": 0}, 8),
    ("epi-chain-256x128", _epi_reg(T256x128), 256, 32, 256, {"gemm_cfg": 3}, 0),
    ("epi-chain-128x128", _epi_reg(T128), 128, 32, 384, {"gemm_cfg": 3}, 0),
    ("epi-chain-128x64", _epi_reg(T128x64), 384, 48, 192, {"gemm_cfg": 3}, 4),
    ("epi-chain-64x64", _epi_reg(T64), 192, 32, 192, {"gemm_cfg": 3}, 0),
    ("epi-64-blocks", _epi_reg(T64), 512, 16, 512, {"gemm_cfg": 1}, 0),             # 64 blocks: the two-level ticket (md_ticket_last2)
    ("epi-chain-64x64-k80", _epi_reg(T64), 64, 80, 320, {"gemm_cfg": 6}, 0),
]
EPI_SENTINEL = 0xA5


def _epi_call(A, W, bias, a_pad=0, a_off=0, b_pad=0, mask_pad=0, mask_off=0, bias_off=0, a_t=False):
    """mask, sum = matmul_bias_relu_sum(A, W, bias) on views of poisoned bases; mask and sum pre-filled with 0xA5 bytes."""
    M, K = A.shape
    N = W.shape[1]
    rng = np.random.default_rng(9)
    fa, oa, sa = _place(A[None], a_t, Op(pad=a_pad, off=a_off), rng)
    fb, ob, sb = _place(W[None], False, Op(pad=b_pad), rng)
    da = nd.asarray(fa)._view(oa, (M, K), sa[1:])
    db = nd.asarray(fb)._view(ob, (K, N), sb[1:])
    dbias = nd.asarray(np.concatenate([np.full(bias_off, np.nan, f32), bias, np.full(4, np.nan, f32)]))._view(bias_off, (N,), (1,))
    mbase = nd.asarray(np.full(mask_off + M * (N + mask_pad) + 16, EPI_SENTINEL, dtype=np.uint8).view(np.bool_))
    dmask = mbase._view(mask_off, (M, N), (N + mask_pad, 1))
    dsum = nd.asarray(np.full(4, EPI_SENTINEL, dtype=np.uint8).view(f32))
    refused = False
    try:
        nd._lib().matmul_bias_relu_sum(da.desc(), db.desc(), dbias.desc(), dmask.desc(), dsum._view(0, (), ()).desc())
    except ValueError:
        refused = True
    mraw, sraw = mbase.get().view(np.uint8), dsum.get()
    if refused:         # untouched: every byte of the mask's base and of the sum still holds the sentinel
        assert (mraw == EPI_SENTINEL).all() and (sraw.view(np.uint8) == EPI_SENTINEL).all()
        return None, None
    idx = mask_off + np.arange(M)[:, None] * (N + mask_pad) + np.arange(N)[None, :]
    outside = np.ones(mraw.size, dtype=bool)
    outside[idx] = False
    assert (mraw[outside] == EPI_SENTINEL).all() and (sraw.view(np.uint8)[4:] == EPI_SENTINEL).all()
    return mraw[idx], sraw[0]


def _plain_product(A, W):
    M, N = A.shape[0], W.shape[1]
    da, db, dc = nd.asarray(A[None]), nd.asarray(W[None]), nd.asarray(np.full((1, M, N), np.nan, dtype=f32))
    nd._lib().matmul(da.desc(), db.desc(), dc.desc())
    return dc.get()[0]


@_twins([x[0] for x in EPI])
def _epilogue(case, mdopt, on_gpu):
    """Integer data with a half-integer bias: mask and sum exact. Float data: the mask equals (a @ b + bias > 0) computed from the
    library's own plain product under the same options, bit for bit, and the sum lies within (tile elements + tiles) u sum(relu) of
    float64 (the CPU double sums all M N terms in one chain: M N u). Identical rows of `a` with bias = -(row of the plain
    product): every pre-activation is exactly 0 if and only if the epilogue's accumulators carry the plain product's bits — the
    mask is all False and the sum is 0. Everything three times, interleaved: the tickets are back at zero."""
    id_, reaches, M, K, N, opts, a_pad = next(x for x in EPI if x[0] == case)
    e = Entry(id_, reaches, f32, M, K, N, opts={"gemm_peel": 0, "gemm_repack": 0, **opts})
    _set_opts(e, mdopt)
    rng = np.random.default_rng([len(TABLE), 13, [x[0] for x in EPI].index(case)])
    vals = np.array([-3, -1, 1, 3], dtype=f32)
    Ai, Wi = rng.choice(vals, (M, K)), rng.choice(vals, (K, N))
    bi = (rng.integers(-20, 20, N) + 0.5).astype(f32)
    zi = Ai.astype(np.float64) @ Wi.astype(np.float64) + bi
    assert 2 * np.abs(zi).sum() < 2 ** 24                     # every partial sum of the relu terms is a multiple of 1/2 below 2^23: exact
    Af, Wf = rng.standard_normal((M, K)).astype(f32), rng.standard_normal((K, N)).astype(f32)
    bf = rng.standard_normal(N).astype(f32)
    Cf = _plain_product(Af, Wf)
    zf = Cf + bf                                              # float32, as the epilogue adds it
    Ar = np.ascontiguousarray(np.broadcast_to(Af[:1], (M, K)))
    Cr = _plain_product(Ar, Wf)
    assert (Cr == Cr[:1]).all()
    t = tuple(int(v) for v in reaches.split("<")[1].split(",")[:2])
    terms = (t[0] * t[1] + (M // t[0]) * (N // t[1])) if on_gpu else M * N
    first = {}
    for rep in range(3):
        for name, (A, W, b) in (("int", (Ai, Wi, bi)), ("float", (Af, Wf, bf)), ("cancel", (Ar, Wf, -Cr[0]))):
            mask, total = _epi_call(A, W, b, a_pad=a_pad)
            assert first.setdefault(name, (mask.tobytes(), total.tobytes())) == (mask.tobytes(), total.tobytes()), (case, name, rep)
            if rep:
                continue
            if name == "int":
                np.testing.assert_array_equal(mask, (zi > 0).astype(np.uint8), err_msg=case)
                assert total == np.maximum(zi, 0).sum(), (case, total)
            elif name == "float":
                wrong = int((mask != (zf > 0)).sum())
                assert wrong == 0, (case, f"{wrong} mask bytes differ from (plain product + bias > 0)")
                ref = np.maximum(zf.astype(np.float64), 0).sum()
                ratio = abs(float(total) - ref) / (terms * 2.0 ** -24 * ref)
                _RATIOS[f"{reaches} | relu sum, bound (tile elements + tiles) u sum(relu)"] = ratio
                assert ratio <= 1.0, (case, ratio)
            else:
                assert not mask.any() and total == 0, (case, int(mask.sum()), float(total), "the epilogue's accumulators are not the plain product's bits")


test_epilogue, test_epilogue_gpu = _epilogue

# what mdhip_matmul_bias_relu_sum refuses with MDHIP_EVALUE; `both`: the CPU double refuses it as well (it keeps the shape rules only)
EPI_REFUSALS = [
    ("M-not-64", dict(M=96 + 8), True), ("N-not-16", dict(N=128 + 8), True), ("K-not-16", dict(K=40), True), ("K-8", dict(K=8), True),
    ("no-tile-divides", dict(M=96), True),
    ("a-off-16B", dict(a_off=1), False), ("a-row-stride-odd", dict(a_pad=1), False), ("b-row-stride-odd", dict(b_pad=2), False),
    ("a-column-major", dict(a_t=True), False), ("mask-row-stride", dict(mask_pad=16), False), ("mask-off-16B", dict(mask_off=4), False),
    # the plain product would sum in another order than the fused kernel could (found by test_epilogue's cancel check on the device:
    # a register-staged epilogue under a direct-to-LDS plain product set 8256 of 20480 mask bytes that `a @ b + bias > 0` does not)
    ("plain-is-dma-k48", dict(M=128, K=48, N=256, opts={"gemm_cfg": 0}), False),
    ("plain-is-dma-ragged-tile", dict(M=192, K=64, N=128, opts={"gemm_cfg": 0}), False),
    ("plain-is-dma-k80-w8", dict(M=64, K=80, N=320, opts={"gemm_cfg": 7}), False),
    ("plain-is-split-k", dict(M=64, K=1024, N=64), False),
    ("plain-is-long-k", dict(M=64, K=8192, N=64), False),
]


@_twins([x[0] for x in EPI_REFUSALS])
def _epilogue_refusals(case, mdopt, on_gpu):
    """Every refusal returns MDHIP_EVALUE (ValueError) and leaves mask and sum untouched. The CPU double keeps the shape rules only (it
    has no alignment, no kernel families to refuse): there the other cases must be COMPUTED right on the same views — which proves the
    views and references of this test."""
    _, kw, both = next(x for x in EPI_REFUSALS if x[0] == case)
    kw = dict(kw)
    M, K, N = kw.pop("M", 128), kw.pop("K", 32), kw.pop("N", 128)
    _set_opts(Entry(case, "refused", f32, M, K, N, opts={"gemm_peel": 0, "gemm_repack": 0, **kw.pop("opts", {})}), mdopt)
    rng = np.random.default_rng(14)
    A, W, b = rng.standard_normal((M, K)).astype(f32), rng.standard_normal((K, N)).astype(f32), rng.standard_normal(N).astype(f32)
    mask, total = _epi_call(A, W, b, **kw)
    if on_gpu or both:
        assert mask is None, (case, "was not refused")
        return
    z = A.astype(np.float64) @ W.astype(np.float64) + b
    far = np.abs(z) > 1e-4                                  # (float32 chain against float64: entries within rounding of 0 may flip)
    assert mask is not None and np.array_equal(mask.astype(bool)[far], (z > 0)[far])
    assert abs(float(total) - np.maximum(z, 0).sum()) <= 1e-5 * np.abs(z).sum()


test_epilogue_refusals, test_epilogue_refusals_gpu = _epilogue_refusals
