"""Opt-in lazy fusion of elementwise chains.

With ``MDHIP_LAZY=1`` (or ``ndarray.set_lazy(True)``) an elementwise backend
call does not launch: it returns a DeviceArray that carries an expression tree.
The tree grows while further elementwise calls consume it and is evaluated in
ONE pass by libmdhip's expression interpreter (``mdhip_vm_eval``) — or folded
into a reduction (``mdhip_vm_reduce``: full reduce, the reduce-to-shape
column sum of the broadcast-gradient path, or a reduction over the trailing
axes: per-row statistics) — when something needs the bytes:
a view, a matmul, a gather, an in-place write, a D2H copy. The tape above is
untouched; it simply sees arrays.

Default is eager (one kernel per backend call, the reference's execution model),
and bench.py reports the eager figure unless ``--lazy`` is given.

Bounds of a fused program (include/mdhip.h): 48 instructions, 8 distinct leaf
arrays, operand stack depth 4. Operators whose operand is a leaf array or a
constant carry it inside the instruction, so a chain costs one instruction per
operator. A tree that would exceed the bounds materialises its larger operand
first. Values are computed in ONE float type per program (float32 or float64 —
whatever NumPy's loop resolution gave each op); bool results travel as 0/1.
Integer loops are never fused, and neither are loops whose dtype is storage-only
itself (float16 + float16, int8 * int8) — except, behind a switch of its own
(``MDHIP_LAZY_F16=1`` / ``ndarray.set_lazy_float16(True)``), float16 loops: they are
recorded into a float32 program whose instructions carry MDHIP_VM_RND16, so every
recorded call rounds its value to binary16 once, as NumPy's half loops and the eager
kernels (csrc/narrow.hip) do. That is not ``astype(float32 chain, float16)``, which
rounds once at the end.

A LEAF may have any of the twelve dtypes: an operand of a float32 / float64 loop
is read in its own storage type (float16, int8/16, uint8/16/32/64, as bool, int32
and int64 always were) and converted on load — NumPy's cast of the operand to the
loop dtype. ``astype(narrow array, float32 | float64)`` is such a leaf by itself
(a pending array whose expression is the LEAF node: consumers read the narrow bytes
and the float copy exists only if its bytes are needed), and
``astype(pending float chain, float16)`` stores the chain's value as float16 in the
same pass (``mdhip_vm_eval`` with a float16 ``out``: one rounding to nearest even).

Behind another switch (``MDHIP_LAZY_ROWS=1`` / ``ndarray.set_lazy_rows(True)``) a chain continues PAST a reduction over the
trailing axes: ``max(x, -1, keepdims=True)`` stays pending as a ROWRED node, and a chain over the same rows that consumes it
(``exp(x - m) / sum(exp(x - m))``) is emitted as a STAGED program (include/mdhip.h) — every distinct ROWRED node one stage that
ends in MDHIP_VM_ROWRED, its uses MDHIP_VM_SRC_ROW operands — which one generated kernel evaluates with the row held in
registers. Where the library refuses such a program (the CPU double always does) the nodes are materialised by the route the
switch-off code takes and the chain is emitted again with them as leaves.
"""
from __future__ import annotations

from . import _capi
from ._capi import VM_BINARY, VM_PUSH, VM_ROWRED, VM_SRC_CONST, VM_SRC_LEAF, VM_SRC_ROW, VM_SRC_STACK, VM_UNARY, VM_WHERE, vm_ctrl

LEAF, CONST, UNARY, BINARY, WHERE, GEMM, ROWRED = range(7)
MAX_INSTR, MAX_LEAVES, MAX_DEPTH, MAX_ROWS = 44, 8, 4, _capi.VM_ROW_REGS


class Expr:
    """Node of a pending expression. `cdt` is the program's float type code (F32/F64);
    `n` / `depth` are the instruction count and stack need of its emitted form. `r16`: the node is a recorded
    float16 call with a float16 result — its instruction rounds the value through binary16 (MDHIP_VM_RND16).
    `rows`: the ROWRED nodes BELOW this node, {id: node} in dependency order (None: none) — each is a stage of the emitted
    program, so `n` counts a ROWRED operand as the one-instruction operand it is and cost() adds the stages.
    A ROWRED node (rowred() below) has args = (child, shape, mask, row length) — the RECORDED expression of the operand, never the
    operand array itself: the node's value must not depend on what is written into that array later —, `value` None
    while it is pending and the concrete (.., 1) array once something materialised it — from then on it is emitted as a leaf —
    and `users`, weak references to the pending arrays whose programs contain it."""

    __slots__ = ("kind", "code", "args", "n", "depth", "leaves", "cdt", "owner", "r16", "rows", "value", "users")

    def __init__(self, kind, code, args, n, depth, leaves, cdt, r16=False, rows=None):
        self.kind, self.code, self.args = kind, code, args
        self.n, self.depth, self.leaves, self.cdt, self.r16, self.rows = n, depth, leaves, cdt, r16, rows
        self.owner = None  # weakref to the pending DeviceArray this node is the value of (set by DeviceArray._pending)


def leaf(arr, cdt):
    return Expr(LEAF, 0, arr, 1, 1, {id(arr): arr}, cdt)


def const(value, cdt):
    return Expr(CONST, 0, float(value), 1, 1, {}, cdt)


def gemm(a, b, cdt):
    """A deferred matrix product a @ b (both concrete 2-D arrays). Not an interpreter instruction: the array that
    carries it materialises through the GEMM kernel, and enters elementwise programs as a LEAF — which lets the
    reduction of `where(a @ b + bias > 0, a @ b + bias, 0)` be recognised and run in the GEMM's epilogue."""
    return Expr(GEMM, 0, (a, b), 1, 1, {}, cdt)


def rowred(child, code, shape, mask, n_red, cdt):
    """reduce(child) over the trailing axes `mask` of `shape`, keepdims, not launched: a row register of the programs that
    consume it. (`rows` holds the nodes below only — a node in its own table would be a reference cycle.)"""
    e = Expr(ROWRED, code, (child, shape, mask, n_red), 1, 1, child.leaves, cdt, False, _rows_below((child,)))
    e.value, e.users = None, []
    return e


def _rows_below(parts):
    rows = None
    for p in parts:
        if p.rows is not None or p.kind == ROWRED:
            if rows is None:
                rows = {}
            if p.rows:
                rows.update(p.rows)
            if p.kind == ROWRED:
                rows[id(p)] = p
    return rows


def live_rows(e):
    """the ROWRED nodes of e (e itself included) that nothing has materialised yet, in dependency order"""
    out = [r for r in e.rows.values() if r.value is None] if e.rows else []
    if e.kind == ROWRED and e.value is None:
        out.append(e)
    return out


def cost(e):
    """(instructions, leaf arrays, row registers) of e's emitted form; the leaf count is an upper bound once a node below has
    been materialised (its stage's leaves are still counted, next to the array that took its place)."""
    if not e.rows:
        return e.n, len(e.leaves), 0
    n, regs, settled = e.n, 0, 0
    for r in e.rows.values():
        if r.value is None:
            n += r.args[0].n + 1
            regs += 1
        elif id(r.value) not in e.leaves:
            settled += 1
    return n, len(e.leaves) + settled, regs


def _simple(e) -> bool:
    return e.kind == LEAF or e.kind == CONST or e.kind == ROWRED


def combine(kind, code, parts, cdt, r16=False):
    leaves = {}
    for p in parts:
        if p.leaves:
            leaves.update(p.leaves)
    rows = _rows_below(parts)
    if rows is not None:
        e = _combine(kind, code, parts, cdt, r16, leaves)
        e.rows = rows
        return e
    return _combine(kind, code, parts, cdt, r16, leaves)


def _combine(kind, code, parts, cdt, r16, leaves):
    if kind == UNARY:
        (a,) = parts
        return Expr(kind, code, (a,), a.n + 1, a.depth, leaves, cdt, r16)
    if kind == BINARY:
        a, b = parts
        sa, sb = _simple(a), _simple(b)
        if sa and sb:
            if a.kind == CONST and b.kind == CONST:      # two immediates: push one, fuse the other
                n, depth = 2, 1
            else:
                n, depth = 1, 1
        elif sb:
            n, depth = a.n + 1, a.depth
        elif sa:
            n, depth = b.n + 1, b.depth
        else:
            n, depth = a.n + b.n + 1, max(a.depth, b.depth + 1)
        return Expr(kind, code, (a, b), n, depth, leaves, cdt, r16)
    c, a, b = parts  # WHERE: all three go through the stack
    n = c.n + a.n + b.n + 1
    depth = max(c.depth, a.depth + 1, b.depth + 2)
    return Expr(kind, code, (c, a, b), n, depth, leaves, cdt)


def fits(e: Expr) -> bool:
    if e.rows:
        # (a register counts as a leaf as well: whenever its node is materialised it becomes one, in every program that holds it,
        # and a program that fitted when it was recorded must still fit then)
        n, leaves, regs = cost(e)
        return n <= MAX_INSTR and e.depth <= MAX_DEPTH and leaves + regs <= MAX_LEAVES and regs <= MAX_ROWS
    return e.n <= MAX_INSTR and e.depth <= MAX_DEPTH and len(e.leaves) <= MAX_LEAVES


class _Emitter:
    """Postfix emission state. A plain object with methods — NOT nested recursive closures,
    which would form a reference cycle and keep the leaf arrays (HBM blocks) alive until
    Python's cyclic GC runs."""

    __slots__ = ("ctrl", "imm", "leaves", "leaf_ix", "regs")

    def __init__(self):
        self.ctrl, self.imm, self.leaves, self.leaf_ix, self.regs = [], [], [], {}, {}

    def src(self, x):
        """(source kind, leaf index, immediate) of a simple operand."""
        if x.kind == LEAF or x.kind == ROWRED:
            arr = x.args
            if x.kind == ROWRED:
                if x.value is None:
                    return VM_SRC_ROW, self.regs[id(x)], 0.0   # a row register, written by the node's stage
                arr = x.value
            k = id(arr)
            ix = self.leaf_ix.get(k)
            if ix is None:
                ix = self.leaf_ix[k] = len(self.leaves)
                self.leaves.append(arr)
            return VM_SRC_LEAF, ix, 0.0
        return VM_SRC_CONST, 0, x.args

    def stage(self, r):
        """the stage of the pending ROWRED node r: its child's value, reduced over the row into the next register"""
        self.walk(r.args[0])
        k = self.regs[id(r)] = len(self.regs)
        self.put(vm_ctrl(VM_ROWRED, r.code, 0, 0, 0, k), float(r.args[3]))

    def put(self, word, value=0.0):
        self.ctrl.append(word)
        self.imm.append(value)

    def walk(self, x):
        if _simple(x):
            s, l, v = self.src(x)
            self.put(vm_ctrl(VM_PUSH, 0, 0, 0, s, l), v)
        elif x.kind == UNARY:
            self.walk(x.args[0])
            self.put(vm_ctrl(VM_UNARY, x.code, rnd16=x.r16))
        elif x.kind == BINARY:
            a, b = x.args
            sa, sb = _simple(a), _simple(b)
            if sa and sb and a.kind == CONST and b.kind == CONST:
                self.walk(a)
                s, l, v = self.src(b)
                self.put(vm_ctrl(VM_BINARY, x.code, VM_SRC_STACK, 0, s, l, x.r16), v)
            elif sa and sb:
                s1, l1, v1 = self.src(a)
                s2, l2, v2 = self.src(b)
                self.put(vm_ctrl(VM_BINARY, x.code, s1, l1, s2, l2, x.r16), v1 if s1 == VM_SRC_CONST else v2)
            elif sb:
                self.walk(a)
                s, l, v = self.src(b)
                self.put(vm_ctrl(VM_BINARY, x.code, VM_SRC_STACK, 0, s, l, x.r16), v)
            elif sa:
                self.walk(b)
                s, l, v = self.src(a)
                self.put(vm_ctrl(VM_BINARY, x.code, s, l, VM_SRC_STACK, 0, x.r16), v)
            else:
                self.walk(a)
                self.walk(b)
                self.put(vm_ctrl(VM_BINARY, x.code, VM_SRC_STACK, 0, VM_SRC_STACK, 0, x.r16))
        else:
            for p in x.args:
                self.walk(p)
            self.put(vm_ctrl(VM_WHERE))


def emit(e: Expr):
    """-> (ctrl words, immediates, leaf arrays)."""
    em = _Emitter()
    if e.rows:   # a staged program: every pending ROWRED node below e once, in dependency order, then e as the final stage
        for r in e.rows.values():
            if r.value is None:
                em.stage(r)
    em.walk(e)
    return em.ctrl, em.imm, em.leaves


def build_program(e: Expr, shape):
    ctrl, imm, leaves = emit(e)
    if len(ctrl) > _capi.VM_MAX_INSTR or len(leaves) > _capi.VM_MAX_LEAVES:
        raise ValueError("fused program exceeds the interpreter's limits")
    prog = _capi.VmProgram()
    prog.n_instr, prog.n_leaves, prog.compute_dtype = len(ctrl), len(leaves), e.cdt
    for i, (c, v) in enumerate(zip(ctrl, imm)):
        prog.ctrl[i] = c
        prog.imm[i] = v
    for i, arr in enumerate(leaves):
        prog.leaves[i] = arr.desc(shape)
    return prog, leaves
