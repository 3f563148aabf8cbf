// fusion_jit.inc — run-time specialisation of a recorded expression (included by
// fusion.hip). The interpreter (md_vm.h) is always available; for large arrays the
// same program is turned into straight-line HIP source — the functors of md_ops.h,
// embedded verbatim, applied in program order — compiled once with hiprtc for gfx950
// and cached by signature (float type, instruction words, leaf dtypes, epilogue).
// Constants and geometry stay kernel ARGUMENTS, so changing a scalar or a shape never
// recompiles. Any failure (no libhiprtc, compile error) falls back to the interpreter.
//
// Generated kernels mirror the interpreter's shapes (eval / full reduce / column
// reduce / row reduce) but with the expression inlined: all leaf loads of an element group are
// issued up front as 16-B vector loads, the body is register-only, occupancy is that
// of a plain streaming kernel — i.e. HBM-bound at the fused byte count.
#include <dlfcn.h>

#include <mutex>
#include <sstream>
#include <unordered_map>

namespace jit {

static const char *kOpsSrc =
#include "md_ops_embed.inc"
    ;
static const char *kTicketSrc =   // md_ticket.h: the single-launch finish of RED_ALL / SWEEP
#include "md_ticket_embed.inc"
    ;

struct JLeaf {
  const void *p;
  long long os;
  int is;
  int pad;
};
struct JArgs {
  JLeaf leaf[MDHIP_VM_MAX_LEAVES];
  double imm[MDHIP_VM_MAX_INSTR];
  void *out;
  long long rows, inner;
  long long n_out, n_red, chunk;
  void *outs[4];  // evaluated outputs (EVAL: one per program; SWEEP with store: outs[0])
  long long dq, dr;  // divmod(grid stride in vectors, vectors per row): position advance of the streaming forms
  void *partial;     // RED_ALL / SWEEP: block partials, combined by the block that arrives last (md_ticket.h)
  void *tickets;     // .. and its counters
  long long bo[MDHIP_VM_MAX_LEAVES];  // batched column reductions: per leaf, the elements from one batch (blockIdx.y) to the next
};
// the axes form of EVAL (three / four collapsed axes): extents of the two inner outer axes and, per leaf, its three outer strides
struct JAxArgs : JArgs {
  long long e1, e2;
  long long st[MDHIP_VM_MAX_LEAVES][3];
};

// ---- hiprtc through dlopen (no link-time dependency) ---------------------------------
typedef struct _hiprtcProgram *rtcProgram;
static struct Rtc {
  void *h = nullptr;
  bool tried = false;
  int (*Create)(rtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*Compile)(rtcProgram, int, const char **) = nullptr;
  int (*GetCodeSize)(rtcProgram, size_t *) = nullptr;
  int (*GetCode)(rtcProgram, char *) = nullptr;
  int (*GetLogSize)(rtcProgram, size_t *) = nullptr;
  int (*GetLog)(rtcProgram, char *) = nullptr;
  int (*Destroy)(rtcProgram *) = nullptr;
} RTC;

static bool rtc_load() {
  if (RTC.tried) return RTC.h != nullptr;
  RTC.tried = true;
  for (const char *n : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
    RTC.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (RTC.h) break;
  }
  if (!RTC.h) return false;
  RTC.Create = (decltype(RTC.Create))dlsym(RTC.h, "hiprtcCreateProgram");
  RTC.Compile = (decltype(RTC.Compile))dlsym(RTC.h, "hiprtcCompileProgram");
  RTC.GetCodeSize = (decltype(RTC.GetCodeSize))dlsym(RTC.h, "hiprtcGetCodeSize");
  RTC.GetCode = (decltype(RTC.GetCode))dlsym(RTC.h, "hiprtcGetCode");
  RTC.GetLogSize = (decltype(RTC.GetLogSize))dlsym(RTC.h, "hiprtcGetProgramLogSize");
  RTC.GetLog = (decltype(RTC.GetLog))dlsym(RTC.h, "hiprtcGetProgramLog");
  RTC.Destroy = (decltype(RTC.Destroy))dlsym(RTC.h, "hiprtcDestroyProgram");
  if (!RTC.Create || !RTC.Compile || !RTC.GetCodeSize || !RTC.GetCode || !RTC.Destroy) {
    RTC.h = nullptr;
    return false;
  }
  return true;
}

// ---- source generation ------------------------------------------------------------------
static const char *unary_expr(int op) {
  switch (op) {
    case MDHIP_U_ABS: return "UAbs::apply(x)";
    case MDHIP_U_NEG: return "UNeg::apply(x)";
    case MDHIP_U_SIGN: return "USign::apply(x)";
    case MDHIP_U_CEIL: return "UCeil::apply(x)";
    case MDHIP_U_FLOOR: return "UFloor::apply(x)";
    case MDHIP_U_SIN: return "USin::apply(x)";
    case MDHIP_U_COS: return "UCos::apply(x)";
    case MDHIP_U_TAN: return "UTan::apply(x)";
    case MDHIP_U_SINH: return "USinh::apply(x)";
    case MDHIP_U_COSH: return "UCosh::apply(x)";
    case MDHIP_U_TANH: return "UTanh::apply(x)";
    case MDHIP_U_EXP: return "UExp::apply(x)";
    case MDHIP_U_LOG: return "ULog::apply(x)";
    case MDHIP_U_SQRT: return "USqrt::apply(x)";
    case MDHIP_U_LOGICAL_NOT: return "(T)(x == (T)0)";
    case MDHIP_U_ISNAN: return "(T)(x != x)";
  }
  return "x";
}
static const char *binary_expr(int op) {
  switch (op) {
    case MDHIP_B_ADD: return "a + b";
    case MDHIP_B_SUB: return "a - b";
    case MDHIP_B_MUL: return "a * b";
    case MDHIP_B_TRUE_DIV: return "a / b";
    case MDHIP_B_FLOOR_DIV: return "BFloorDiv::apply(a, b)";
    case MDHIP_B_MOD: return "BMod::apply(a, b)";
    case MDHIP_B_POW: return "BPow::apply(a, b)";
    case MDHIP_B_MAXIMUM: return "BMaximum::apply(a, b)";
    case MDHIP_B_MINIMUM: return "BMinimum::apply(a, b)";
    case MDHIP_B_EQ: return "(T)(a == b)";
    case MDHIP_B_NE: return "(T)(a != b)";
    case MDHIP_B_LT: return "(T)(a < b)";
    case MDHIP_B_LE: return "(T)(a <= b)";
    case MDHIP_B_GT: return "(T)(a > b)";
    case MDHIP_B_GE: return "(T)(a >= b)";
    case MDHIP_B_LAND: return "(T)((a != (T)0) && (b != (T)0))";
    case MDHIP_B_LOR: return "(T)((a != (T)0) || (b != (T)0))";
    case MDHIP_B_LXOR: return "(T)((a != (T)0) != (b != (T)0))";
  }
  return "a";
}
// the type a leaf is read in (jcvt converts it to T): every dtype by name — a default that widened would make a narrower leaf's
// vector load run past the array. An unknown code (md_vm_check refuses it) names no type: the source does not compile.
static const char *storage_name(int dt) {
  switch (dt) {
    case MDHIP_BOOL: return "uint8_t";   // truth values: jcvt gives x != 0
    case MDHIP_I32: return "int32_t";
    case MDHIP_I64: return "int64_t";
    case MDHIP_F32: return "float";
    case MDHIP_F64: return "double";
    case MDHIP_F16: return "f16";
    case MDHIP_I8: return "int8_t";
    case MDHIP_U8: return "ju8";         // a uint8 VALUE
    case MDHIP_I16: return "int16_t";
    case MDHIP_U16: return "uint16_t";
    case MDHIP_U32: return "uint32_t";
    case MDHIP_U64: return "uint64_t";
  }
  return "jno_such_dtype";
}
static const char *reduce_name(int op) {
  switch (op) {
    case MDHIP_R_SUM: return "RSum";
    case MDHIP_R_PROD: return "RProd";
    case MDHIP_R_MAX: return "RMax";
  }
  return "RMin";
}

// ---- what one generated kernel is ----------------------------------------------------------------
// How a leaf is read is a compile-time property of the generated kernel (part of the cache key), so
// that the loads of one trip are unconditional and issue back to back:
//   LM_VEC    unit inner stride: one vector load per group of 4 elements (16 B; 8 / 4 B for 2- / 1-byte leaves, 2 x 16 B for 8-byte ones) (RED_ROWS: also the row-invariant
//             vector, at row stride 0 — every row re-reads it from the caches)
//   LM_ROWB   inner stride 0, row stride != 0 (a column broadcast): one scalar load per row
//   LM_CONST  ONE device element behind a stride-0 view (the backward seed): read once in the prologue
//   (the axes form of EVAL: LM_VEC at r0*s0 + r1*s1 + r2*s2 + c, LM_ROWB one load per group at the outer offset, LM_CONST when
//    the three outer strides are 0 as well)
//   LM_ROWINV (sweep kernels only) unit inner stride, row stride 0 (the bias row): the lane's column
//             vectors are loaded once, before the row loop
enum { LM_VEC = 0, LM_ROWB = 1, LM_CONST = 2, LM_ROWINV = 3 };
enum Kind { EVAL = 0, RED_ALL = 1, RED_COLS = 2, SWEEP = 3, RED_ROWS = 4, ROWS_STAGED = 5 };

struct Spec {
  int kind = EVAL;
  int n = 1;                        // programs = outputs of an EVAL (1..4); 1 for the reductions
  const mdhip_vm_program *pr[4] = {};
  int leaf_map[4][MDHIP_VM_MAX_LEAVES] = {};
  int imm_slot[4][MDHIP_VM_MAX_INSTR] = {};
  int n_leaves = 0, n_imm = 0;
  int leaf_dtype[MDHIP_VM_MAX_LEAVES] = {};
  int leaf_mode[MDHIP_VM_MAX_LEAVES] = {};
  bool f32 = true, out_bool = false, nt = false;
  bool out_f16 = false;             // EVAL, one output: the value is rounded once to binary16 and stored as such (8-byte vectors)
  bool nt_store = false;            // non-temporal stores although the loads are cached (SWEEP with store, see sweep_cols)
  int rop = MDHIP_R_SUM;
  bool store = false;               // SWEEP: also write the evaluated value (eval + reduce-to-shape in one pass)
  int Q = 1, RU = 1;                // SWEEP: column vectors per lane (row = Q x 1024 elements), rows per trip
  int U = 2;                        // EVAL / RED_ALL: independent vector groups per lane and trip
  int axes = 0;                     // EVAL: 0 the (rows, inner) form | 3, 4 that many collapsed axes (fusion.hip's axes_geometry)
  bool wide = false;                // EVAL over axes: 64-bit vector index (2^31 vectors and more), else 32-bit
  int NV = 0;                       // RED_ROWS: 1, 2, 4, 8 vector groups per lane, a wave per row | 0 a block per row
                                    // ROWS_STAGED (a staged program: its stages are cut at the ROWREDs of pr[0]): 1, 2, 4, 8
  int G = 0;                        // ROWS_STAGED: 0 a wave per row (NV) | 3 .. 8 a block per row, that many vector groups per lane (NV is 0)
  bool batch = false;               // RED_COLS / SWEEP: `outer` independent (n_red, n_out) problems, the batch on blockIdx.y (a middle axis reduced)
};

static void spec_single(Spec *S, const mdhip_vm_program *pr) {
  S->n = 1;
  S->pr[0] = pr;
  S->n_leaves = pr->n_leaves;
  S->n_imm = pr->n_instr;
  S->f32 = pr->compute_dtype == MDHIP_F32;
  for (int l = 0; l < pr->n_leaves; ++l) { S->leaf_map[0][l] = l; S->leaf_dtype[l] = pr->leaves[l].dtype; }
  for (int i = 0; i < pr->n_instr; ++i) S->imm_slot[0][i] = i;
}
// leaf read modes from the collapsed (rows, inner) geometry
static void spec_modes(Spec *S, const MdVmDev &D, int64_t rows) {
  for (int l = 0; l < S->n_leaves; ++l) {
    const bool is = D.leaf[l].is != 0;
    const int64_t os = D.leaf[l].os;
    if (is) S->leaf_mode[l] = (S->kind == SWEEP && os == 0 && rows > 1) ? LM_ROWINV : LM_VEC;
    else S->leaf_mode[l] = (os == 0 || rows == 1) ? LM_CONST : LM_ROWB;
  }
}

// which leaves feed sin / cos DIRECTLY (the d/dx sin(x) = cos(x) pattern of a backward pass): their
// values are computed once per element ahead of the program bodies — ONE sincos when both occur
struct TrigUse {
  bool s[MDHIP_VM_MAX_LEAVES] = {}, c[MDHIP_VM_MAX_LEAVES] = {};
};
static void scan_trig(const mdhip_vm_program *pr, const int *leaf_map, TrigUse *tu) {
  std::vector<int> st;  // merged leaf slot when the value IS that leaf, else -1
  for (int pc = 0; pc < pr->n_instr; ++pc) {
    const uint32_t c = pr->ctrl[pc];
    const uint32_t k = MD_VM_KIND(c), op = MD_VM_OP(c), ls = MD_VM_LS(c), rs = MD_VM_RS(c);
    if (k == MDHIP_VM_PUSH) {
      st.push_back(rs == MDHIP_VM_SRC_LEAF ? leaf_map[MD_VM_RL(c)] : -1);
    } else if (k == MDHIP_VM_UNARY) {
      const int top = st.back();
      if (top >= 0 && op == MDHIP_U_SIN) tu->s[top] = true;
      if (top >= 0 && op == MDHIP_U_COS) tu->c[top] = true;
      st.back() = -1;
    } else if (k == MDHIP_VM_BINARY) {
      if (rs == MDHIP_VM_SRC_STACK) st.pop_back();
      if (ls == MDHIP_VM_SRC_STACK) st.pop_back();
      st.push_back(-1);
    } else {
      st.pop_back(); st.pop_back(); st.pop_back();
      st.push_back(-1);
    }
  }
}

// body<k>(): program k as scalar SSA over one element; leaf values (and their hoisted sin / cos) arrive as arguments
// (a staged program: body<b> is the stage [pc0, pc1) of program k, and the n_regs row registers written before it arrive as r0, ..)
static std::string gen_body(const Spec &S, int k, const TrigUse &tu, int b = -1, int pc0 = 0, int pc1 = -1, int n_regs = 0) {
  const mdhip_vm_program *pr = S.pr[k];
  if (b < 0) b = k;
  if (pc1 < 0) pc1 = pr->n_instr;
  std::ostringstream o;
  o << "__device__ __forceinline__ T body" << b << "(const JArgs &A";
  for (int l = 0; l < S.n_leaves; ++l) o << ", const T l" << l;
  for (int r = 0; r < n_regs; ++r) o << ", const T r" << r;
  for (int l = 0; l < S.n_leaves; ++l) {
    if (tu.s[l]) o << ", const T sn" << l;
    if (tu.c[l]) o << ", const T cs" << l;
  }
  o << ") {\n";
  std::vector<std::string> st;
  auto operand = [&](uint32_t src, uint32_t leaf, int pc) -> std::string {
    if (src == MDHIP_VM_SRC_LEAF) return "l" + std::to_string(S.leaf_map[k][leaf]);
    if (src == MDHIP_VM_SRC_ROW) return "r" + std::to_string(leaf);
    o << "  const T c" << pc << " = (T)A.imm[" << S.imm_slot[k][pc] << "];\n";
    return "c" + std::to_string(pc);
  };
  for (int pc = pc0; pc < pc1; ++pc) {
    const uint32_t c = pr->ctrl[pc];
    const uint32_t kd = MD_VM_KIND(c), op = MD_VM_OP(c), ls = MD_VM_LS(c), rs = MD_VM_RS(c);
    const bool r16 = (c & MDHIP_VM_RND16) != 0;  // the instruction's value goes through binary16 (md_vm.h: md_vm_round16)
    static const char *const rnd[2] = {"(", "jr16("};
    if (kd == MDHIP_VM_PUSH) {
      st.push_back(operand(rs, MD_VM_RL(c), pc));
    } else if (kd == MDHIP_VM_UNARY) {
      std::string x = st.back();
      st.pop_back();
      if ((op == MDHIP_U_SIN || op == MDHIP_U_COS) && x.size() >= 2 && x[0] == 'l' && x.find_first_not_of("0123456789", 1) == std::string::npos &&
          (op == MDHIP_U_SIN ? tu.s : tu.c)[std::stoi(x.substr(1))]) {
        const std::string h = (op == MDHIP_U_SIN ? "sn" : "cs") + x.substr(1);  // hoisted
        if (r16) {  // the hoisted value is shared with unflagged uses: round it where this instruction takes it
          o << "  const T t" << pc << " = jr16(" << h << ");\n";
          st.push_back("t" + std::to_string(pc));
        } else {
          st.push_back(h);
        }
        continue;
      }
      o << "  T t" << pc << "; { const T x = " << x << "; t" << pc << " = " << rnd[r16] << unary_expr(op) << "); }\n";
      st.push_back("t" + std::to_string(pc));
    } else if (kd == MDHIP_VM_BINARY) {
      std::string a, b;
      if (rs == MDHIP_VM_SRC_STACK) { b = st.back(); st.pop_back(); } else b = operand(rs, MD_VM_RL(c), pc);
      if (ls == MDHIP_VM_SRC_STACK) { a = st.back(); st.pop_back(); } else a = operand(ls, MD_VM_LL(c), pc);
      o << "  T t" << pc << "; { const T a = " << a << ", b = " << b << "; t" << pc << " = " << rnd[r16] << binary_expr(op) << "); }\n";
      st.push_back("t" + std::to_string(pc));
    } else {
      std::string z = st.back(); st.pop_back();
      std::string y = st.back(); st.pop_back();
      std::string cnd = st.back(); st.pop_back();
      o << "  const T t" << pc << " = (" << cnd << " != (T)0) ? " << y << " : " << z << ";\n";
      st.push_back("t" + std::to_string(pc));
    }
  }
  o << "  return " << st.back() << ";\n}\n";
  return o.str();
}

static void gen_prelude(std::ostringstream &o, const Spec &S, const std::string &kname) {
  o << kOpsSrc << "\n";
  if (S.kind == RED_ALL || S.kind == SWEEP) o << kTicketSrc << "\n";
  // The bodies below are straight-line source: `a * b` followed by `a + b` would be contracted into ONE fused multiply-add — one
  // rounding where the eager kernels, the interpreter (switch dispatch: nothing to contract across) and NumPy round twice. From
  // here on nothing is contracted. The functors above keep the mode the eager kernels compile them in: the compiler's expansion
  // of logf ends in a contracted multiply-add, so -ffp-contract=off for the whole unit would change log(x) in the last bit
  // (tests/test_elementwise_accuracy.py: paths, chains. Seen on the device with that flag: log(x) from a generated kernel differed
  // from the eager kernel's in 12258 of 65536 float32 arguments by one ulp, e.g. log(FLT_MAX) = 0x42b17217 against 0x42b17218.)
  // This relies on hiprtc's default contraction mode, fast-honor-pragmas: under a global -ffp-contract=fast the backend fuses
  // whatever the pragma says. Only the GPU twins of the chain tests notice that — the CPU double has no generated kernels.
  o << "#pragma clang fp contract(off)\n";
  o << "#define KNAME " << kname << "\n";
  o << "constexpr bool JNT = " << (S.nt ? "true" : "false") << ";  // non-temporal 16-B loads (streams larger than the Infinity Cache)\n";
  o << "constexpr bool JNT_ST = " << ((S.nt || S.nt_store) ? "true" : "false") << ";  // non-temporal 16-B stores\n";
  o << "typedef " << (S.f32 ? "float" : "double") << " T;\n";
  o << "typedef " << (S.out_bool ? "b8" : S.out_f16 ? "f16" : "T") << " To;\n";
  o << "typedef " << reduce_name(S.rop) << " R;\n";
  o << R"(
template <class S, int N> struct alignas(sizeof(S) * N > 16 ? 16 : sizeof(S) * N) JVec { S v[N]; };
struct JLeaf { const void *p; long long os; int is; int pad; };
struct JArgs { JLeaf leaf[8]; double imm[48]; void *out; long long rows, inner; long long n_out, n_red, chunk; void *outs[4]; long long dq, dr; void *partial; void *tickets; long long bo[8]; };
struct JAxArgs : JArgs { long long e1, e2; long long st[8][3]; };
template <class S> __device__ __forceinline__ T jcvt(S x) { return (T)x; }
template <> __device__ __forceinline__ T jcvt<uint8_t>(uint8_t x) { return (T)(x != 0); }
struct ju8 { uint8_t v; };
template <> __device__ __forceinline__ T jcvt<ju8>(ju8 x) { return (T)x.v; }
template <> __device__ __forceinline__ T jcvt<f16>(f16 x) { return md_cast<T>(x); }
__device__ __forceinline__ T jr16(T x) { return md_cast<T>(md_cast<f16>(x)); }  // MDHIP_VM_RND16: through binary16, nearest even
template <class V> __device__ __forceinline__ V jld(const V *p) {
  if constexpr (JNT && sizeof(V) == 16) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4 t = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(p));
    V v; __builtin_memcpy(&v, &t, 16); return v;
  } else { return *p; }
}
template <class V> __device__ __forceinline__ void jst(V *p, const V &v) {
  if constexpr (JNT_ST && sizeof(V) == 16) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4 t; __builtin_memcpy(&t, &v, 16);
    __builtin_nontemporal_store(t, reinterpret_cast<i32x4 *>(p));
  } else { *p = v; }
}
// 4 adjacent elements of a unit-stride leaf
template <class S> __device__ __forceinline__ void jloadv(const JLeaf &L, long long row, long long c, T (&d)[4]) {
  JVec<S, 4> v = jld(reinterpret_cast<const JVec<S, 4> *>((const S *)L.p + row * L.os + c));
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = jcvt<S>(v.v[j]);
}
template <class S> __device__ __forceinline__ T jload1(const JLeaf &L, long long off) { return jcvt<S>(((const S *)L.p)[off]); }
__device__ __forceinline__ float jshfl(float v, int d) { return __shfl_down(v, d, 64); }
__device__ __forceinline__ double jshfl(double v, int d) {
  union { double f; int w[2]; } u; u.f = v;
  u.w[0] = __shfl_down(u.w[0], d, 64); u.w[1] = __shfl_down(u.w[1], d, 64);
  return u.f;
}
// (row, column-vector) of vector `gid`, advanced by additions: (dq, dr) = divmod(grid stride, vectors per row) from the host
struct JPos {
  long long row, cv;
  __device__ __forceinline__ void init(const JArgs &A, long long gid, long long nv) {
    row = 0; cv = gid;
    if (A.rows != 1) {
      if ((unsigned long long)gid < 0x100000000ull && (unsigned long long)nv < 0x100000000ull) {
        const unsigned q = (unsigned)gid / (unsigned)nv; row = q; cv = (unsigned)gid - q * (unsigned)nv;
      } else { row = gid / nv; cv = gid - row * nv; }
    }
  }
  __device__ __forceinline__ void advance(const JArgs &A, long long nv) {
    cv += A.dr; row += A.dq;
    if (cv >= nv) { cv -= nv; ++row; }
  }
};
)";
}

// Text fragments that read the leaves: `pro` once per thread (LM_CONST), `vec(row, c, sfx)` the loads of one
// 4-element group (arrays named l<k><sfx>), `trig(sfx)` the hoisted sin / cos of that group, `args(sfx, j)` the body
// arguments for element j of the group, `one(off...)` the single-element forms of the 1-D tail.
struct LeafText {
  const Spec &S;
  const TrigUse &tu;
  static std::string trig_scalar(const std::string &x, const std::string &sn, const std::string &cs, bool s, bool c) {
    if (s && c) return "md_sincos(" + x + ", &" + sn + ", &" + cs + ");";
    if (s) return sn + " = USin::apply(" + x + ");";
    return cs + " = UCos::apply(" + x + ");";
  }
  std::string pro() const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      if (S.leaf_mode[l] != LM_CONST) continue;
      o << "  const T k" << l << " = jload1<" << storage_name(S.leaf_dtype[l]) << ">(A.leaf[" << l << "], 0);\n";
      if (tu.s[l] || tu.c[l]) {
        o << "  T ksn" << l << " = (T)0, kcs" << l << " = (T)0; " << trig_scalar("k" + std::to_string(l), "ksn" + std::to_string(l), "kcs" + std::to_string(l), tu.s[l], tu.c[l]) << "\n";
      }
    }
    return o.str();
  }
  // loads of one group; `modes`: bit mask of leaf modes to emit (so that invariant leaves can be emitted apart)
  std::string vec(const std::string &row, const std::string &c, const std::string &sfx, unsigned modes, const char *ind = "    ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (!((modes >> m) & 1u)) continue;
      const char *St = storage_name(S.leaf_dtype[l]);
      if (m == LM_VEC) o << ind << "T l" << l << sfx << "[4]; jloadv<" << St << ">(A.leaf[" << l << "], " << row << ", " << c << ", l" << l << sfx << ");\n";
      else if (m == LM_ROWINV) o << ind << "T l" << l << sfx << "[4]; jloadv<" << St << ">(A.leaf[" << l << "], 0, " << c << ", l" << l << sfx << ");\n";
      else if (m == LM_ROWB) o << ind << "const T l" << l << sfx << " = jload1<" << St << ">(A.leaf[" << l << "], (" << row << ") * A.leaf[" << l << "].os);\n";
    }
    return o.str();
  }
  // loads of one group of the axes form: the position is in r0<sfx> (four axes only), r1<sfx>, r2<sfx>, c<sfx>
  std::string vec_axes(const std::string &sfx, const char *ind = "    ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (m != LM_VEC && m != LM_ROWB) continue;
      const char *St = storage_name(S.leaf_dtype[l]);
      const std::string L = "A.st[" + std::to_string(l) + "]";
      const std::string off = (S.axes == 4 ? "r0" + sfx + " * " + L + "[0] + " : std::string()) + "r1" + sfx + " * " + L + "[1] + r2" + sfx + " * " + L + "[2]";
      if (m == LM_VEC) o << ind << "T l" << l << sfx << "[4]; jloadv<" << St << ">(A.leaf[" << l << "], 0, " << off << " + c" << sfx << ", l" << l << sfx << ");\n";
      else o << ind << "const T l" << l << sfx << " = jload1<" << St << ">(A.leaf[" << l << "], " << off << ");\n";
    }
    return o.str();
  }
  // The same loads in two halves, for the software-pipelined sweep: `raw` issues them into registers of the STORAGE type
  // (declared by `decl`, assigned a batch ahead), `cvt` makes the T arrays the bodies read — the conversion is the first
  // use, so the wait for a batch sits in front of ITS compute phase and not behind the issue of the next one.
  std::string decl(const std::string &sfx, unsigned modes, const char *ind = "  ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (!((modes >> m) & 1u)) continue;
      const char *St = storage_name(S.leaf_dtype[l]);
      if (m == LM_VEC) o << ind << "JVec<" << St << ", 4> r" << l << sfx << ";\n";
      else if (m == LM_ROWB) o << ind << St << " r" << l << sfx << ";\n";
    }
    return o.str();
  }
  std::string raw(const std::string &row, const std::string &c, const std::string &sfx, unsigned modes, const char *ind = "    ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (!((modes >> m) & 1u)) continue;
      const char *St = storage_name(S.leaf_dtype[l]);
      if (m == LM_VEC) o << ind << "r" << l << sfx << " = jld(reinterpret_cast<const JVec<" << St << ", 4> *>((const " << St << " *)A.leaf[" << l << "].p + (" << row << ") * A.leaf[" << l << "].os + " << c << "));\n";
      else if (m == LM_ROWB) o << ind << "r" << l << sfx << " = ((const " << St << " *)A.leaf[" << l << "].p)[(" << row << ") * A.leaf[" << l << "].os];\n";
    }
    return o.str();
  }
  std::string cvt(const std::string &sfx, unsigned modes, const char *ind = "    ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (!((modes >> m) & 1u)) continue;
      const char *St = storage_name(S.leaf_dtype[l]);
      if (m == LM_VEC) o << ind << "T l" << l << sfx << "[4];\n" << ind << "#pragma unroll\n" << ind << "for (int j = 0; j < 4; ++j) l" << l << sfx << "[j] = jcvt<" << St << ">(r" << l << sfx << ".v[j]);\n";
      else if (m == LM_ROWB) o << ind << "const T l" << l << sfx << " = jcvt<" << St << ">(r" << l << sfx << ");\n";
    }
    return o.str();
  }
  std::string trig(const std::string &sfx, unsigned modes, const char *ind = "    ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (!(tu.s[l] || tu.c[l]) || !((modes >> m) & 1u)) continue;
      const std::string L = "l" + std::to_string(l) + sfx, sn = "sn" + std::to_string(l) + sfx, cs = "cs" + std::to_string(l) + sfx;
      if (m == LM_VEC || m == LM_ROWINV) {
        o << ind << "T " << sn << "[4], " << cs << "[4];\n" << ind << "#pragma unroll\n" << ind << "for (int j = 0; j < 4; ++j) { " << sn << "[j] = (T)0; " << cs
          << "[j] = (T)0; " << trig_scalar(L + "[j]", sn + "[j]", cs + "[j]", tu.s[l], tu.c[l]) << " }\n";
      } else if (m == LM_ROWB) {
        o << ind << "T " << sn << " = (T)0, " << cs << " = (T)0; " << trig_scalar(L, sn, cs, tu.s[l], tu.c[l]) << "\n";
      }
    }
    return o.str();
  }
  // (`rowb`: the suffix of the LM_ROWB leaves where they are loaded apart from the vector groups — once per row in RED_ROWS)
  std::string args(const std::string &sfx, const std::string &j, const char *rowb = nullptr) const {
    std::ostringstream o;
    const std::string rsfx = rowb ? std::string(rowb) : sfx;
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      if (m == LM_CONST) o << ", k" << l;
      else if (m == LM_ROWB) o << ", l" << l << rsfx;
      else o << ", l" << l << sfx << "[" << j << "]";
    }
    for (int l = 0; l < S.n_leaves; ++l) {
      const int m = S.leaf_mode[l];
      const bool arr = m == LM_VEC || m == LM_ROWINV;
      const std::string pre = m == LM_CONST ? "k" : "";
      const std::string sf = m == LM_CONST ? std::string() : m == LM_ROWB ? rsfx : sfx;
      if (tu.s[l]) o << ", " << pre << "sn" << l << sf << (arr ? "[" + j + "]" : "");
      if (tu.c[l]) o << ", " << pre << "cs" << l << sf << (arr ? "[" + j + "]" : "");
    }
    return o.str();
  }
  // the single element i of a 1-D launch (rows == 1: only LM_VEC and LM_CONST leaves exist)
  std::string one(const char *ind = "      ") const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) {
      if (S.leaf_mode[l] == LM_CONST) continue;
      o << ind << "const T e" << l << " = jload1<" << storage_name(S.leaf_dtype[l]) << ">(A.leaf[" << l << "], i);\n";
      if (tu.s[l] || tu.c[l])
        o << ind << "T esn" << l << " = (T)0, ecs" << l << " = (T)0; " << trig_scalar("e" + std::to_string(l), "esn" + std::to_string(l), "ecs" + std::to_string(l), tu.s[l], tu.c[l]) << "\n";
    }
    return o.str();
  }
  std::string args_one() const {
    std::ostringstream o;
    for (int l = 0; l < S.n_leaves; ++l) o << (S.leaf_mode[l] == LM_CONST ? ", k" : ", e") << l;
    for (int l = 0; l < S.n_leaves; ++l) {
      const char *pre = S.leaf_mode[l] == LM_CONST ? "k" : "e";
      if (tu.s[l]) o << ", " << pre << "sn" << l;
      if (tu.c[l]) o << ", " << pre << "cs" << l;
    }
    return o.str();
  }
};

constexpr unsigned LM_ALL = 0xFu;
// (Spec::U: independent vector groups per lane and trip in the streaming forms EVAL / RED_ALL)

static std::string kind_tag(const Spec &S) {
  switch (S.kind) {
    case EVAL: {
      const std::string form = S.axes ? "evalaxes" : "eval";
      return S.n > 1 ? form + std::to_string(S.n) : (S.out_bool && !S.axes ? "evalb" : S.out_f16 ? form + "h" : form);
    }
    case RED_ALL: return "redall";
    case RED_COLS: return S.batch ? "redcolsb" : "redcols";
    case RED_ROWS: return S.NV ? "redrowsw" + std::to_string(S.NV) : "redrowsb";
    case ROWS_STAGED: return S.G ? "rowsresb" + std::to_string(S.G) : "rowsres" + std::to_string(S.NV);
  }
  return S.store ? "evalcols" : S.batch ? "sweepb" : "sweepcols";
}

static std::string gen_source(const Spec &S, const std::string &kname) {
  TrigUse tu;   // (a staged program hoists nothing: a held sin / cos would cost registers through every stage)
  if (S.kind != ROWS_STAGED)
    for (int k = 0; k < S.n; ++k) scan_trig(S.pr[k], S.leaf_map[k], &tu);
  std::ostringstream o;
  gen_prelude(o, S, kname);
  if (S.kind != ROWS_STAGED)
    for (int k = 0; k < S.n; ++k) o << gen_body(S, k, tu);
  const LeafText LT{S, tu};
  auto emit_outputs = [&](const std::string &sfx, const std::string &off, const char *ind) {
    std::ostringstream e;
    for (int k = 0; k < S.n; ++k) {
      e << ind << "{ JVec<To, 4> o;\n" << ind << "#pragma unroll\n" << ind << "  for (int j = 0; j < 4; ++j) o.v[j] = md_cast<To>(body" << k << "(A" << LT.args(sfx, "j") << "));\n"
        << ind << "  jst(reinterpret_cast<JVec<To, 4> *>((To *)A.outs[" << k << "] + " << off << "), o); }\n";
    }
    return e.str();
  };
  // batched column reductions (a middle axis reduced: the program seen as (outer, n_red, n_out)): block row blockIdx.y works on
  // its own (n_red, n_out) problem — every leaf's base and `out` move on by the batch's offset, the rest of the kernel is the 2-D one
  auto batch_pro = [&]() {
    std::ostringstream e;
    e << "  const long long bt = blockIdx.y;\n";
    for (int l = 0; l < S.n_leaves; ++l)
      e << "  A.leaf[" << l << "].p = (const " << storage_name(S.leaf_dtype[l]) << " *)A.leaf[" << l << "].p + bt * A.bo[" << l << "];\n";
    e << "  A.out = (T *)A.out + bt * A.n_out;\n";
    return e.str();
  };
  if (S.kind == EVAL && S.axes) {
    // Three / four collapsed axes (k_vm_eval_axes with the expression inlined): a lane takes U vectors of four per trip, the outer
    // position of each from two or three divisions of its vector index — 32-bit, or 64-bit from 2^31 vectors on: the host's choice.
    // The output is dense, so its offset is the vector index itself.
    o << "typedef " << (S.wide ? "long long" : "unsigned") << " I;\n"
         "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JAxArgs A) {\n"
         "  const I nv = (I)(A.inner >> 2), total = (I)A.rows * nv, e1 = (I)A.e1, e2 = (I)A.e2;\n"
         "  const I gid = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x, gs = (I)gridDim.x * (I)blockDim.x;\n"
      << LT.pro() << "  I v = gid;\n";
    auto position = [&](const std::string &sfx, const std::string &vx) {
      std::ostringstream e;
      e << "    const I v" << sfx << " = " << vx << ", w" << sfx << " = v" << sfx << " / nv, q" << sfx << " = w" << sfx << " / e2;\n"
        << "    const long long off" << sfx << " = (long long)v" << sfx << " << 2, c" << sfx << " = (long long)(v" << sfx << " - w" << sfx << " * nv) << 2, r2" << sfx
        << " = (long long)(w" << sfx << " - q" << sfx << " * e2);\n";
      if (S.axes == 4)
        e << "    const I t" << sfx << " = q" << sfx << " / e1;\n    const long long r0" << sfx << " = (long long)t" << sfx << ", r1" << sfx << " = (long long)(q" << sfx << " - t"
          << sfx << " * e1);\n";
      else
        e << "    const long long r1" << sfx << " = (long long)q" << sfx << ";\n";
      return e.str();
    };
    o << "  for (; v + " << (S.U - 1) << " * gs < total; v += " << S.U << " * gs) {\n";
    for (int u = 0; u < S.U; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << position(sfx, "v + " + std::to_string(u) + " * gs") << LT.vec_axes(sfx);
    }
    for (int u = 0; u < S.U; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << LT.trig(sfx, LM_ALL) << emit_outputs(sfx, "off" + sfx, "    ");
    }
    o << "  }\n  for (; v < total; v += gs) {\n" << position("_t", "v") << LT.vec_axes("_t") << LT.trig("_t", LM_ALL) << emit_outputs("_t", "off_t", "    ") << "  }\n}\n";
  } else if (S.kind == EVAL) {
    o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
         "  const long long nv = A.inner >> 2, total = A.rows * nv;\n"
         "  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gs = (long long)gridDim.x * blockDim.x;\n"
      << LT.pro() << "  JPos P; P.init(A, gid, nv);\n  long long v = gid;\n";
    // main trips: S.U groups, every load ahead of the first use
    o << "  for (; v + " << (S.U - 1) << " * gs < total; v += " << S.U << " * gs) {\n";
    for (int u = 0; u < S.U; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << "    const long long off" << sfx << " = P.row * A.inner + (P.cv << 2);\n" << LT.vec("P.row", "(P.cv << 2)", sfx, LM_ALL) << "    P.advance(A, nv);\n";
    }
    for (int u = 0; u < S.U; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << LT.trig(sfx, LM_ALL) << emit_outputs(sfx, "off" + sfx, "    ");
    }
    o << "  }\n  for (; v < total; v += gs) {\n    const long long off = P.row * A.inner + (P.cv << 2);\n"
      << LT.vec("P.row", "(P.cv << 2)", "", LM_ALL) << "    P.advance(A, nv);\n" << LT.trig("", LM_ALL) << emit_outputs("", "off", "    ") << "  }\n";
    o << "  if (A.rows == 1) {\n    const long long i = (nv << 2) + gid;\n    if (i < A.inner) {\n" << LT.one();
    for (int k = 0; k < S.n; ++k) o << "      ((To *)A.outs[" << k << "])[i] = md_cast<To>(body" << k << "(A" << LT.args_one() << "));\n";
    o << "    }\n  }\n}\n";
  } else if (S.kind == RED_ALL) {
    o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
         "  __shared__ T smem[4];\n  __shared__ unsigned last_flag;\n"
         "  const long long nv = A.inner >> 2, total = A.rows * nv;\n"
         "  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gs = (long long)gridDim.x * blockDim.x;\n"
      << LT.pro() << "  JPos P; P.init(A, gid, nv);\n  long long v = gid;\n"
         "  T a[" << S.U << "][4];\n#pragma unroll\n  for (int u = 0; u < " << S.U << "; ++u)\n#pragma unroll\n    for (int j = 0; j < 4; ++j) a[u][j] = R::template identity<T>();\n";
    o << "  for (; v + " << (S.U - 1) << " * gs < total; v += " << S.U << " * gs) {\n";
    for (int u = 0; u < S.U; ++u) o << LT.vec("P.row", "(P.cv << 2)", "_" + std::to_string(u), LM_ALL) << "    P.advance(A, nv);\n";
    for (int u = 0; u < S.U; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << LT.trig(sfx, LM_ALL) << "#pragma unroll\n    for (int j = 0; j < 4; ++j) a[" << u << "][j] = R::combine(a[" << u << "][j], body0(A" << LT.args(sfx, "j") << "));\n";
    }
    o << "  }\n  for (; v < total; v += gs) {\n" << LT.vec("P.row", "(P.cv << 2)", "", LM_ALL) << "    P.advance(A, nv);\n" << LT.trig("", LM_ALL)
      << "#pragma unroll\n    for (int j = 0; j < 4; ++j) a[0][j] = R::combine(a[0][j], body0(A" << LT.args("", "j") << "));\n  }\n";
    o << "  T acc = R::template identity<T>();\n#pragma unroll\n  for (int u = 0; u < " << S.U << "; ++u) acc = R::combine(acc, R::combine(R::combine(a[u][0], a[u][1]), R::combine(a[u][2], a[u][3])));\n";
    o << "  if (A.rows == 1) {\n    const long long i = (nv << 2) + gid;\n    if (i < A.inner) {\n" << LT.one() << "      acc = R::combine(acc, body0(A" << LT.args_one() << "));\n    }\n  }\n";
    o << R"(#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = R::combine(acc, jshfl(acc, d));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) smem[w] = acc;
  __syncthreads();
  // block partials -> the block that arrives last sums them in index order (md_ticket.h): no finishing launch
  T *partial = (T *)A.partial;
  if (threadIdx.x == 0) md_st_sc1(partial + blockIdx.x, R::combine(R::combine(smem[0], smem[1]), R::combine(smem[2], smem[3])));
  const bool last = gridDim.x >= 64 ? md_ticket_last2((unsigned *)A.tickets, blockIdx.x, gridDim.x, &last_flag)
                                    : md_ticket_last((unsigned *)A.tickets, gridDim.x, &last_flag);
  if (!last) return;
  acc = md_fold_partials<R>(partial, gridDim.x);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = R::combine(acc, jshfl(acc, d));
  if (lane == 0) smem[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ((T *)A.out)[0] = R::combine(R::combine(smem[0], smem[1]), R::combine(smem[2], smem[3]));
}
)";
  } else if (S.kind == RED_ROWS) {
    // (n_out rows, n_red columns) reduced over the columns; row-broadcast leaves (the m of exp(x - m)) cost one scalar load per row
    const unsigned vecm = 1u << LM_VEC, rowb = 1u << LM_ROWB;
    auto combine = [&](const std::string &acc, const std::string &sfx, const char *ind) {
      return std::string(ind) + "#pragma unroll\n" + ind + "for (int j = 0; j < 4; ++j) " + acc + "[j] = R::combine(" + acc + "[j], body0(A" + LT.args(sfx, "j", "_r") + "));\n";
    };
    if (S.NV) {
      // short rows (reduce.hip's k_reduce_rows_wave with the expression inlined): a wave per row, four rows per block, lane l
      // takes vector groups l + 64 g, g < NV, all loads issued before the first use; a group past the end of the row re-reads
      // group 0 and stays out of the combine. Four accumulators (one per vector component), merged pairwise, then the wave tree.
      o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
           "  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;\n"
           "  const long long row = (long long)blockIdx.x * 4 + w;\n"
           "  if (row >= A.n_out) return;  // (whole waves: no barrier below)\n"
           "  const long long nv = A.n_red >> 2;\n"
        << LT.pro() << LT.vec("row", "0", "_r", rowb, "  ") << LT.trig("_r", rowb, "  ");
      for (int g = 0; g < S.NV; ++g) {
        const std::string sfx = "_" + std::to_string(g);
        o << "  const bool ok" << sfx << " = lane + " << 64 * g << " < nv;\n"
          << "  const long long c" << sfx << " = (ok" << sfx << " ? (long long)(lane + " << 64 * g << ") : 0ll) << 2;\n"
          << LT.vec("row", "c" + sfx, sfx, vecm, "  ");
      }
      o << "  T a[4];\n#pragma unroll\n  for (int j = 0; j < 4; ++j) a[j] = R::template identity<T>();\n";
      for (int g = 0; g < S.NV; ++g) {
        const std::string sfx = "_" + std::to_string(g);
        o << "  if (ok" << sfx << ") {\n" << LT.trig(sfx, vecm, "    ") << combine("a", sfx, "    ") << "  }\n";
      }
      o << R"(  T acc = R::combine(R::combine(a[0], a[1]), R::combine(a[2], a[3]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = R::combine(acc, jshfl(acc, d));
  if (lane == 0) ((T *)A.out)[row] = acc;
}
)";
    } else {
      // long rows: a block per row, 256 lanes stride the row's vector groups with two in flight (as RED_ALL), wave tree, four
      // partials through LDS, one store
      o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
           "  __shared__ T smem[4];\n"
           "  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;\n"
           "  const long long row = blockIdx.x, nv = A.n_red >> 2;\n"
        << LT.pro() << LT.vec("row", "0", "_r", rowb, "  ") << LT.trig("_r", rowb, "  ")
        << "  T a[2][4];\n#pragma unroll\n  for (int u = 0; u < 2; ++u)\n#pragma unroll\n    for (int j = 0; j < 4; ++j) a[u][j] = R::template identity<T>();\n"
           "  long long v = threadIdx.x;\n"
           "  for (; v + 256 < nv; v += 512) {\n"
        << LT.vec("row", "(v << 2)", "_0", vecm) << LT.vec("row", "((v + 256) << 2)", "_1", vecm)
        << LT.trig("_0", vecm) << combine("a[0]", "_0", "    ") << LT.trig("_1", vecm) << combine("a[1]", "_1", "    ")
        << "  }\n  if (v < nv) {\n" << LT.vec("row", "(v << 2)", "_t", vecm) << LT.trig("_t", vecm) << combine("a[0]", "_t", "    ") << "  }\n";
      o << R"(  T acc = R::combine(R::combine(R::combine(a[0][0], a[1][0]), R::combine(a[0][1], a[1][1])), R::combine(R::combine(a[0][2], a[1][2]), R::combine(a[0][3], a[1][3])));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = R::combine(acc, jshfl(acc, d));
  if (lane == 0) smem[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ((T *)A.out)[row] = R::combine(R::combine(smem[0], smem[1]), R::combine(smem[2], smem[3]));
}
)";
    }
  } else if (S.kind == ROWS_STAGED) {
    // A staged program (include/mdhip.h: stage, ROWRED -> r0, stage, ROWRED -> r1, .., final stage) on the geometry of the wave-per-row
    // reduction above: a wave per row, four rows per block, lane l holds the vector groups l + 64 g, g < NV, of every vector leaf —
    // loaded once, all loads ahead of the first use. Each stage is evaluated on the held values and combined EXACTLY as
    // redrowsw<NV> combines: four accumulators over the groups in order, merged pairwise, the 64-lane tree; lane 0's result then goes
    // to every lane (through a scalar register: a row statistic costs no vector register). The final stage is evaluated on the same
    // values and stored as 16-byte vectors. One read of the operands, one write, no statistic in memory.
    const unsigned vecm = 1u << LM_VEC, rowb = 1u << LM_ROWB;
    const mdhip_vm_program *pr = S.pr[0];
    std::vector<int> cut;     // pc of every ROWRED
    for (int pc = 0; pc < pr->n_instr; ++pc)
      if (MD_VM_KIND(pr->ctrl[pc]) == MDHIP_VM_ROWRED) cut.push_back(pc);
    const int ns = (int)cut.size();
    for (int s = 0; s <= ns; ++s) o << gen_body(S, 0, tu, s, s ? cut[s - 1] + 1 : 0, s < ns ? cut[s] : pr->n_instr, s);
    o << R"(__device__ __forceinline__ float jbcast(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double jbcast(double v) {
  union { double f; int w[2]; } u; u.f = v;
  u.w[0] = __builtin_amdgcn_readfirstlane(u.w[0]); u.w[1] = __builtin_amdgcn_readfirstlane(u.w[1]);
  return u.f;
}
)";
    // S.G (rows longer than a wave holds): a BLOCK per row, the grid exactly n_out blocks, lane t of 256 holds the groups t + 256 g,
    // g < G. Each stage combines EXACTLY as redrowsb above combines: its loop puts lane t's group g into the accumulator set
    // a[g & 1] in ascending g (the pair loop takes g, g + 1; its tail is an even group, into a[0]) — unrolled here over the held
    // groups — then the same merge of the two sets, the 64-lane tree, and the four wave partials through LDS as (s0 . s1) . (s2 . s3).
    // Every lane forms that last combine itself, from the stage's own four LDS words after ONE barrier (same operands, same order:
    // same bits), so no second barrier guards the words against the next stage. No lane returns early: the grid has no idle block,
    // and a lane without a live group still takes part in every tree and barrier.
    const int NG = S.G ? S.G : S.NV, LW = S.G ? 256 : 64;   // groups per lane, lanes per row
    const char *ln = S.G ? "(int)threadIdx.x" : "lane";
    if (S.G)
      o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
           "  __shared__ T smem[" << (ns > 0 ? ns : 1) << "][4];\n"
           "  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;\n"
           "  const long long row = blockIdx.x, nv = A.n_red >> 2;  // (the grid is n_out blocks: every block has a row)\n";
    else
      o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
           "  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;\n"
           "  const long long row = (long long)blockIdx.x * 4 + w;\n"
           "  if (row >= A.n_out) return;  // (whole waves: no barrier below, and every lane of a live wave is active)\n"
           "  const long long nv = A.n_red >> 2;\n";
    o << LT.pro() << LT.vec("row", "0", "_r", rowb, "  ");
    for (int g = 0; g < NG; ++g) {
      const std::string sfx = "_" + std::to_string(g);
      o << "  const bool ok" << sfx << " = " << ln << " + " << LW * g << " < nv;\n"
        << "  const long long c" << sfx << " = (ok" << sfx << " ? (long long)(" << ln << " + " << LW * g << ") : 0ll) << 2;\n"
        << LT.vec("row", "c" + sfx, sfx, vecm, "  ");
    }
    auto regs = [](int n) {
      std::string r;
      for (int k = 0; k < n; ++k) r += ", r" + std::to_string(k);
      return r;
    };
    if (S.G) for (int s = 0; s < ns; ++s) {
      const std::string R = reduce_name((int)MD_VM_OP(pr->ctrl[cut[s]]));
      auto cmb = [&](const std::string &x, const std::string &y) { return R + "::combine(" + x + ", " + y + ")"; };
      o << "  T r" << s << ";\n  {\n    T a[2][4];\n#pragma unroll\n    for (int u = 0; u < 2; ++u)\n#pragma unroll\n      for (int j = 0; j < 4; ++j) a[u][j] = " << R << "::template identity<T>();\n";
      for (int g = 0; g < NG; ++g) {
        const std::string sfx = "_" + std::to_string(g), acc = "a[" + std::to_string(g & 1) + "][j]";
        o << "    if (ok" << sfx << ") {\n#pragma unroll\n      for (int j = 0; j < 4; ++j) " << acc << " = " << cmb(acc, "body" + std::to_string(s) + "(A" + LT.args(sfx, "j", "_r") + regs(s) + ")") << ";\n    }\n";
      }
      o << "    T acc = " << cmb(cmb(cmb("a[0][0]", "a[1][0]"), cmb("a[0][1]", "a[1][1]")), cmb(cmb("a[0][2]", "a[1][2]"), cmb("a[0][3]", "a[1][3]"))) << ";\n"
           "#pragma unroll\n    for (int d = 32; d > 0; d >>= 1) acc = " << R << "::combine(acc, jshfl(acc, d));\n"
           "    if (lane == 0) smem[" << s << "][w] = acc;\n    __syncthreads();\n"
           "    r" << s << " = jbcast(" << cmb(cmb("smem[" + std::to_string(s) + "][0]", "smem[" + std::to_string(s) + "][1]"), cmb("smem[" + std::to_string(s) + "][2]", "smem[" + std::to_string(s) + "][3]"))
        << ");  // every lane holds the row's value: through a scalar register\n  }\n";
    }
    else for (int s = 0; s < ns; ++s) {
      const std::string R = reduce_name((int)MD_VM_OP(pr->ctrl[cut[s]]));
      o << "  T r" << s << ";\n  {\n    T a[4];\n#pragma unroll\n    for (int j = 0; j < 4; ++j) a[j] = " << R << "::template identity<T>();\n";
      for (int g = 0; g < S.NV; ++g) {
        const std::string sfx = "_" + std::to_string(g);
        o << "    if (ok" << sfx << ") {\n#pragma unroll\n      for (int j = 0; j < 4; ++j) a[j] = " << R << "::combine(a[j], body" << s << "(A" << LT.args(sfx, "j", "_r") << regs(s) << "));\n    }\n";
      }
      o << "    T acc = " << R << "::combine(" << R << "::combine(a[0], a[1]), " << R << "::combine(a[2], a[3]));\n"
           "#pragma unroll\n    for (int d = 32; d > 0; d >>= 1) acc = " << R << "::combine(acc, jshfl(acc, d));\n"
           "    r" << s << " = jbcast(acc);  // lane 0 holds the row's value: to every lane\n  }\n";
    }
    for (int g = 0; g < NG; ++g) {
      const std::string sfx = "_" + std::to_string(g);
      o << "  if (ok" << sfx << ") {\n    JVec<T, 4> o;\n#pragma unroll\n    for (int j = 0; j < 4; ++j) o.v[j] = body" << ns << "(A" << LT.args(sfx, "j", "_r") << regs(ns) << ");\n"
        << "    jst(reinterpret_cast<JVec<T, 4> *>((T *)A.outs[0] + row * A.n_red + c" << sfx << "), o);\n  }\n";
    }
    o << "}\n";
  } else if (S.kind == RED_COLS) {
    // tiled: block = 64 column groups x 4 row lanes, rows split over gridDim.y; two rows in flight per lane
    // (batched: gridDim.y is the batch, rows unsplit — the form below the strips kernel's floor of 512 reduced rows)
    o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
         "  __shared__ T smem[3][64][4];\n"
         "  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;\n"
         "  const long long col = ((long long)blockIdx.x * 64 + cx) * 4;\n"
      << (S.batch ? "  const long long s = 0, r0 = 0, r1 = A.n_red;  // unsplit: the grid's second dimension is the batch\n" + batch_pro()
                  : std::string("  const long long s = blockIdx.y, r0 = s * A.chunk;\n"
                                "  long long r1 = r0 + A.chunk;\n  if (r1 > A.n_red) r1 = A.n_red;\n"))
      << LT.pro() <<
         "  T a[2][4];\n#pragma unroll\n  for (int u = 0; u < 2; ++u)\n#pragma unroll\n    for (int j = 0; j < 4; ++j) a[u][j] = R::template identity<T>();\n"
         "  if (col < A.n_out) {\n    const long long c = col;\n    long long row = r0 + ry;\n    for (; row + 4 < r1; row += 8) {\n"
      << LT.vec("row", "c", "_0", LM_ALL, "      ") << LT.vec("(row + 4)", "c", "_1", LM_ALL, "      ");
    for (int u = 0; u < 2; ++u) {
      const std::string sfx = "_" + std::to_string(u);
      o << LT.trig(sfx, LM_ALL, "      ") << "#pragma unroll\n      for (int j = 0; j < 4; ++j) a[" << u << "][j] = R::combine(a[" << u << "][j], body0(A" << LT.args(sfx, "j") << "));\n";
    }
    o << "    }\n    for (; row < r1; row += 4) {\n" << LT.vec("row", "c", "", LM_ALL, "      ") << LT.trig("", LM_ALL, "      ")
      << "#pragma unroll\n      for (int j = 0; j < 4; ++j) a[0][j] = R::combine(a[0][j], body0(A" << LT.args("", "j") << "));\n    }\n  }\n";
    o << R"(  T tot[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tot[j] = R::combine(a[0][j], a[1][j]);
  if (ry > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) smem[ry - 1][cx][j] = tot[j];
  }
  __syncthreads();
  if (ry == 0 && col < A.n_out) {
    JVec<T, 4> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = R::combine(R::combine(tot[j], smem[0][cx][j]), R::combine(smem[1][cx][j], smem[2][cx][j]));
    *reinterpret_cast<JVec<T, 4> *>((T *)A.out + s * A.n_out + col) = o;
  }
}
)";
  } else {
    // SWEEP (strips form, as reduce.hip's k_reduce_cols_strips): grid = NS column strips x NB row bands; a strip is 64 lanes
    // x 4 elements; the four waves of a block and the bands take the rows interleaved (row = band + NB * (wave + 4 i)), so the
    // grid reads one moving window of the operands; RU rows per trip are in flight; row-invariant leaves (the bias) are read
    // once per lane. With `store` the evaluated value is written as well: the elementwise product and its reduce-to-shape
    // cost ONE pass over the operands. Waves merge through LDS, bands through write-through partial rows and a ticket per
    // strip (md_ticket.h): the block that arrives last adds the strip's partial rows in band order — one launch.
    const unsigned inv = 1u << LM_ROWINV;
    o << "extern \"C\" __global__ void __launch_bounds__(256) KNAME(JArgs A) {\n"
         "  __shared__ JVec<T, 4> sm[3][64];\n  __shared__ unsigned last_flag;\n"
         "  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;\n"
         "  const int NB = (int)A.chunk, NS = (int)(gridDim.x / NB);\n"
         "  const int s = blockIdx.x % NS, b = blockIdx.x / NS;\n"
         "  const long long col_raw = ((long long)s * 64 + lane) * 4;\n"
         "  const bool col_ok = col_raw < A.n_out;\n"
         "  const long long c = col_ok ? col_raw : A.n_out - 4;  // lanes past a ragged edge compute a valid group and store nothing\n"
         "  const long long first = b + (long long)NB * w, step = (long long)NB * 4;\n"
         "  const long long nrw = first < A.n_red ? (A.n_red - first + step - 1) / step : 0;  // rows of this wave: first + step * i\n";
    if (S.batch)  // .. and each batch has its own partial rows and its own ticket per strip
      o << batch_pro() << "  A.partial = (T *)A.partial + bt * NB * A.n_out;\n  A.tickets = (unsigned *)A.tickets + bt * NS * MD_TICKET_PAD;\n";
    o << LT.pro() <<
         "  T acc[4];\n#pragma unroll\n  for (int j = 0; j < 4; ++j) acc[j] = R::template identity<T>();\n";
    o << LT.vec("0", "c", "_i", inv, "  ") << LT.trig("_i", inv, "  ");
    const unsigned vecm = 1u << LM_VEC, rowb = 1u << LM_ROWB;
    // rows (i + u) of this wave, u < ru, in two phases; `bs` names the batch's registers ("_a", "_b", "_t")
    auto issue = [&](int ru, const std::string &bs, const char *ind) {
      std::ostringstream e;
      for (int u = 0; u < ru; ++u) {
        const std::string row = "(first + step * (i + " + std::to_string(u) + "))";
        e << LT.raw(row, "0", bs + std::to_string(u), rowb, ind) << LT.raw(row, "c", bs + std::to_string(u), vecm, ind);
      }
      return e.str();
    };
    auto compute = [&](int ru, const std::string &bs, const char *ind) {
      std::ostringstream e;
      for (int u = 0; u < ru; ++u) {
        const std::string sfx = bs + std::to_string(u);
        e << ind << "{\n" << LT.cvt(sfx, rowb | vecm, ind) << LT.trig(sfx, rowb | vecm, ind);
        std::ostringstream a;
        for (int l = 0; l < S.n_leaves; ++l) {
          const int m = S.leaf_mode[l];
          if (m == LM_CONST) a << ", k" << l;
          else if (m == LM_ROWB) a << ", l" << l << sfx;
          else a << ", l" << l << (m == LM_ROWINV ? "_i" : sfx) << "[j]";
        }
        for (int l = 0; l < S.n_leaves; ++l) {
          const int m = S.leaf_mode[l];
          const std::string sf = m == LM_CONST ? "" : (m == LM_ROWINV ? "_i" : sfx);
          const std::string pre = m == LM_CONST ? "k" : "";
          const bool arr = m == LM_VEC || m == LM_ROWINV;
          if (tu.s[l]) a << ", " << pre << "sn" << l << sf << (arr ? "[j]" : "");
          if (tu.c[l]) a << ", " << pre << "cs" << l << sf << (arr ? "[j]" : "");
        }
        e << ind << "  JVec<T, 4> o;\n" << ind << "#pragma unroll\n" << ind << "  for (int j = 0; j < 4; ++j) { const T val = body0(A" << a.str()
          << "); acc[j] = R::combine(acc[j], val); o.v[j] = val; }\n";
        if (S.store)
          e << ind << "  if (col_ok) jst(reinterpret_cast<JVec<T, 4> *>((T *)A.outs[0] + (first + step * (i + " << u << ")) * A.inner + c), o);\n";
        e << ind << "}\n";
      }
      return e.str();
    };
    // Two batches of RU rows in flight (software pipeline): the next batch is issued BEFORE the landed one is consumed —
    // with one wave per SIMD nothing else covers the issue gap, and a batch's stores (vmcnt is in-order on gfx9) would
    // otherwise sit in front of the next batch's loads. A prefetch past the end re-reads the last batch (discarded): no
    // branch; scheduling barriers pin the order, left alone the compiler sinks the prefetch behind the compute.
    const int RU = S.RU;
    for (int u = 0; u < RU; ++u) o << LT.decl("_a" + std::to_string(u), rowb | vecm) << LT.decl("_b" + std::to_string(u), rowb | vecm);
    o << "  const long long nbt = nrw / " << RU << ";\n"
         "  if (nbt > 0) {\n"
         "    { const long long i = 0;\n" << issue(RU, "_a", "      ") << "    }\n"
         "    long long t = 0;\n"
         "    for (; t + 1 < nbt; t += 2) {\n"
         "      { const long long i = (t + 1) * " << RU << ";\n" << issue(RU, "_b", "        ") << "      }\n"
         "      __builtin_amdgcn_sched_barrier(0);\n"
         "      { const long long i = t * " << RU << ";\n" << compute(RU, "_a", "        ") << "      }\n"
         "      __builtin_amdgcn_sched_barrier(0);\n"
         "      { const long long i = (t + 2 < nbt ? t + 2 : nbt - 1) * " << RU << ";\n" << issue(RU, "_a", "        ") << "      }\n"
         "      __builtin_amdgcn_sched_barrier(0);\n"
         "      { const long long i = (t + 1) * " << RU << ";\n" << compute(RU, "_b", "        ") << "      }\n"
         "      __builtin_amdgcn_sched_barrier(0);\n"
         "    }\n"
         "    if (t < nbt) { const long long i = t * " << RU << ";\n" << compute(RU, "_a", "      ") << "    }\n"
         "  }\n"
         "  for (long long i = nbt * " << RU << "; i < nrw; ++i) {\n" << LT.decl("_t0", rowb | vecm, "    ") << issue(1, "_t", "    ") << compute(1, "_t", "    ") << "  }\n";
    o << R"(  JVec<T, 4> mine;
#pragma unroll
  for (int j = 0; j < 4; ++j) mine.v[j] = acc[j];
  if (w > 0) sm[w - 1][lane] = mine;
  __syncthreads();
  if (w == 0) {  // waves 1..3 -> wave 0, in wave order
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) mine.v[j] = R::combine(mine.v[j], sm[k][lane].v[j]);
  }
  T *out = (T *)A.out;
  if (NB == 1) {
    if (w == 0 && col_ok) *reinterpret_cast<JVec<T, 4> *>(out + c) = mine;
    return;
  }
  const __amdgpu_buffer_rsrc_t pr = md_rsrc(A.partial, (unsigned)((long long)NB * A.n_out * (long long)sizeof(T)));
  if (w == 0 && col_ok) md_st16_sc1(pr, (unsigned)(((long long)b * A.n_out + c) * (long long)sizeof(T)), mine);
  if (!md_ticket_last((unsigned *)A.tickets + s * MD_TICKET_PAD, (unsigned)NB, &last_flag)) return;
  // the strip's NB (<= 64) partial rows: wave w takes rows w, w + 4, ..; every load ahead of the first add
  JVec<T, 4> pt[16];
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (w + 4 * k < NB) pt[k] = md_ld16_sc1<JVec<T, 4>>(pr, (unsigned)(((long long)(w + 4 * k) * A.n_out + c) * (long long)sizeof(T)));
#pragma unroll
  for (int j = 0; j < 4; ++j) mine.v[j] = R::template identity<T>();
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (w + 4 * k < NB) {
#pragma unroll
      for (int j = 0; j < 4; ++j) mine.v[j] = R::combine(mine.v[j], pt[k].v[j]);
    }
  if (w > 0) sm[w - 1][lane] = mine;
  __syncthreads();
  if (w == 0 && col_ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) mine.v[j] = R::combine(mine.v[j], sm[k][lane].v[j]);
    *reinterpret_cast<JVec<T, 4> *>(out + c) = mine;
  }
}
)";
  }
  return o.str();
}

static std::string make_key(const Spec &S) {
  std::ostringstream k;
  k << S.kind << ':' << (int)S.f32 << (int)S.out_bool << (int)S.nt << (int)S.nt_store << (int)S.store << ':' << S.rop << ':' << S.Q << ':' << S.RU << ':' << S.U << ':' << S.n << ':' << S.axes << (int)S.wide << ':' << S.NV;
  if (S.batch) k << 'b';
  if (S.G) k << 'g' << S.G;   // (the wave form's key is what it was)
  if (S.out_f16) k << 'h';
  for (int p = 0; p < S.n; ++p) {
    k << '/';
    // whole ctrl words, MDHIP_VM_RND16 (bit 18) included: a program that rounds through binary16 never shares a kernel with its unflagged twin
    for (int i = 0; i < S.pr[p]->n_instr; ++i) k << std::hex << S.pr[p]->ctrl[i] << ',';
    k << '@';
    for (int l = 0; l < S.pr[p]->n_leaves; ++l) k << S.leaf_map[p][l];
  }
  k << '|';
  for (int l = 0; l < S.n_leaves; ++l) k << S.leaf_dtype[l] << S.leaf_mode[l];
  return k.str();
}
// kernel name the profiler shows: what the kernel is + a digest of its signature
static std::string make_name(const Spec &S, const std::string &key) {
  unsigned long long h = 1469598103934665603ull;
  for (unsigned char ch : key) { h ^= ch; h *= 1099511628211ull; }
  char buf[64];
  snprintf(buf, sizeof buf, "k_fused_%s_%06llx", kind_tag(S).c_str(), h & 0xffffffull);
  return buf;
}

// compile only (no device needed): used by the probe entry point and by get()
static int compile(const std::string &src, std::vector<char> *code, std::string *log) {
  if (!rtc_load()) { if (log) *log = "libhiprtc not available"; return -1; }
  rtcProgram prog = nullptr;
  if (RTC.Create(&prog, src.c_str(), "mdhip_fused.hip", 0, nullptr, nullptr) != 0) { if (log) *log = "hiprtcCreateProgram failed"; return -1; }
  // (option jit_verbose = 2: the compiler's resource remarks — registers, scratch, occupancy of the kernel — come back in the log
  // of a successful compilation too: how the probe shows that a form does not spill)
  const bool usage = md_opt(MD_OPT_JIT_VERBOSE) >= 2;
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage"};
  const int rc = RTC.Compile(prog, usage ? 4 : 3, opts);
  if (rc != 0 || usage) {
    if (log && RTC.GetLogSize && RTC.GetLog) {
      size_t n = 0;
      RTC.GetLogSize(prog, &n);
      log->assign(n, '\0');
      if (n) RTC.GetLog(prog, &(*log)[0]);
    }
  }
  if (rc != 0) {
    RTC.Destroy(&prog);
    return -1;
  }
  size_t n = 0;
  RTC.GetCodeSize(prog, &n);
  code->resize(n);
  RTC.GetCode(prog, code->data());
  RTC.Destroy(&prog);
  return 0;
}

struct Entry {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;  // nullptr => known failure, use the interpreter
};
static std::mutex g_mu;
static std::unordered_map<std::string, Entry> g_cache;
static int g_compiled = 0, g_launched = 0;

static int64_t min_elems() { return md_opt(MD_OPT_JIT_MIN); }
static bool enabled() { return md_opt(MD_OPT_JIT) != 0; }

static hipFunction_t get(const Spec &S) {
  const std::string key = make_key(S);
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_cache.find(key);
  if (it != g_cache.end()) return it->second.fn;
  Entry e;
  std::vector<char> code;
  std::string log;
  const std::string name = make_name(S, key);
  if (compile(gen_source(S, name), &code, &log) == 0) {
    if (hipModuleLoadData(&e.mod, code.data()) == hipSuccess && hipModuleGetFunction(&e.fn, e.mod, name.c_str()) == hipSuccess) {
      ++g_compiled;
    } else {
      (void)hipGetLastError();
      e.fn = nullptr;
    }
  } else if (md_opt(MD_OPT_JIT_VERBOSE)) {
    fprintf(stderr, "[mdhip] fused-kernel compilation failed, using the interpreter:\n%s\n", log.c_str());
  }
  g_cache[key] = e;
  return e.fn;
}

template <class Args> static int launch(hipFunction_t fn, Args &A, dim3 grid) {
  size_t sz = sizeof(Args);
  void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  ++g_launched;
  hipEvent_t e0, e1;
  if (md_prof_take(&e0, &e1))   // bench.py attached events: the dispatch carries the kernel's own start / stop timestamps
    return md_hip_check(hipExtModuleLaunchKernel(fn, grid.x * MD_BLOCK, grid.y, 1, MD_BLOCK, 1, 1, 0, md_stream(), nullptr, cfg, e0, e1, 0), "fused kernel launch");
  return md_hip_check(hipModuleLaunchKernel(fn, grid.x, grid.y, 1, MD_BLOCK, 1, 1, 0, md_stream(), nullptr, cfg), "fused kernel launch");
}

// ---- what the launch planners and runners of fusion.hip share -------------------------------------------------------------
// The common part of a Spec for ONE program on the (rows, inner) geometry of D. false: no generated kernel is wanted (option
// jit = 0, or fewer than jit_min elements in all) — the interpreter runs.
static bool spec_for(Spec *S, int kind, const mdhip_vm_program *pr, const MdVmDev &D, int64_t rows, int64_t total, int rop = MDHIP_R_SUM,
                     bool batch = false) {
  if (!enabled() || total < min_elems()) return false;
  S->kind = kind;
  S->batch = batch;
  spec_single(S, pr);
  spec_modes(S, D, rows);
  S->rop = rop;
  return true;
}

// A launch that streams more than this many bytes loads (and an EVAL stores) non-temporally: Spec::nt, part of the kernel's key
constexpr int64_t NT_BYTES = (int64_t)320 << 20;
// What a launch streams through its leaves: `elems` elements of every leaf read with unit inner stride. `row_wise`: only of
// those that also advance from row to row (os != 0) — the forms that walk rows (SWEEP, RED_ROWS) load a row-invariant vector
// once (LM_ROWINV) or re-read it from the caches, the streaming forms (EVAL, RED_ALL) count every vector leaf. On more than one
// row that is exactly SWEEP's LM_VEC, which its launcher used to test; the two predicates are NOT interchangeable: a leaf that
// changes sides changes `nt`, and with it the kernel.
static int64_t streamed_bytes(const MdVmDev &D, int64_t elems, bool row_wise) {
  int64_t bytes = 0;
  for (int l = 0; l < D.n_leaves; ++l)
    if (D.leaf[l].is && (!row_wise || D.leaf[l].os)) bytes += elems * (int64_t)md_dtype_size(D.leaf[l].dtype);
  return bytes;
}

// Kernel arguments: the D.n_leaves leaves as the planner left them in D and n_imm immediates (a single program: one per
// instruction; merged programs: their shared array), everything else 0. Args: JArgs or JAxArgs. (The axes form does not read
// leaf.os; axes_geometry leaves it 0 in D, so it is 0 here as well. In the same way spec_for's spec_modes is idle for the axes
// form: spec_axes sets the mode of every leaf after it.)
template <class Args> static void fill_args(Args *A, const MdVmDev &D, const double *imm, int n_imm) {
  memset(A, 0, sizeof *A);
  for (int l = 0; l < D.n_leaves; ++l) {
    A->leaf[l].p = D.leaf[l].p;
    A->leaf[l].os = D.leaf[l].os;
    A->leaf[l].is = D.leaf[l].is;
  }
  for (int i = 0; i < n_imm; ++i) A->imm[i] = imm[i];
}
// .. the shape group of the reductions over columns or rows
static void args_shape(JArgs *A, int64_t rows, int64_t inner, int64_t n_out, int64_t n_red, int64_t chunk) {
  A->rows = rows; A->inner = inner; A->n_out = n_out; A->n_red = n_red; A->chunk = chunk;
}
// .. and the batch strides of the batched column reductions
static void args_batch(JArgs *A, const VmBatch &B, int n_leaves) {
  for (int l = 0; l < n_leaves; ++l) A->bo[l] = B.bs[l];
}
// Shape of a generated EVAL kernel: vector groups per lane and trip, blocks per CU (options jit_u / jit_blocks force: experiments)
static void eval_shape(Spec *S) {
  const int u = (int)md_opt(MD_OPT_JIT_U);
  S->U = u > 0 ? (u > 4 ? 4 : u) : 2;
}
// Blocks per CU by the number of 16-B streams a lane keeps going (vector leaves + outputs), as the eager kernels choose (8 for one or
// two streams, 4 for three: profiles/r2_ew_grid_ab.log); four and more — cfg3's two-output gradient pass: x, y in, x.grad, y.grad
// out — ran fastest with 2 (two boxes, interleaved rounds: whole sweep 455 -> 422 us and 412 -> 404 us, profiles/r4_jit_shape_ab.txt)
static int eval_blocks(const Spec &S) {
  const int b = (int)md_opt(MD_OPT_JIT_BLOCKS);
  if (b > 0) return b;
  int streams = S.n;
  for (int l = 0; l < S.n_leaves; ++l) streams += S.leaf_mode[l] == LM_VEC;
  return streams >= 4 ? 2 : streams == 3 ? 4 : 8;
}
// geometry of the streaming forms (EVAL / RED_ALL): grid size ..
static int stream_grid(int64_t rows, int64_t inner, int blocks_per_cu = 8) {
  const int64_t nv = inner >> 2;
  const int cap = md_max_blocks();  // (MDHIP_MAX_BLOCKS overrides the per-form choice: experiments)
  return md_grid_for(rows * nv + (rows == 1 ? 4 : 0), MD_BLOCK, cap != MD_NUM_CUS * 8 ? cap : MD_NUM_CUS * blocks_per_cu);
}
// .. and, in the arguments, the position advance per trip of that grid
static void args_stream(JArgs *A, int64_t rows, int64_t inner, int grid) {
  const int64_t nv = inner >> 2, gs = (int64_t)grid * MD_BLOCK;
  A->rows = rows;
  A->inner = inner;
  A->dq = nv > 0 ? gs / nv : 0;
  A->dr = nv > 0 ? gs % nv : 0;
}

static int axes_grid(const Spec &S, const VmAxes &G) {
  const int cap = md_max_blocks();
  return md_grid_for(G.rows * G.nv, MD_BLOCK, cap != MD_NUM_CUS * 8 ? cap : MD_NUM_CUS * eval_blocks(S));
}
// The axes form of EVAL (fusion.hip's axes_geometry passed): read modes from the stride table, index width from the vector count
// (option jit_axes_wide = 1 forces the 64-bit form: tests), non-temporal by the streamed bytes. `out_elem_bytes`: all outputs together.
static void spec_axes(Spec *S, const MdVmDev &D, const VmAxes &G, int64_t out_elem_bytes) {
  const int64_t total = G.rows * G.nv * 4;
  S->axes = G.e0 != 1 ? 4 : 3;
  for (int l = 0; l < S->n_leaves; ++l) {
    if (D.leaf[l].is) S->leaf_mode[l] = LM_VEC;
    else S->leaf_mode[l] = (G.st[l][0] | G.st[l][1] | G.st[l][2]) == 0 ? LM_CONST : LM_ROWB;
  }
  S->nt = total * out_elem_bytes + streamed_bytes(D, total, false) > NT_BYTES;
  eval_shape(S);
  // 32-bit index arithmetic while the largest value the trip loop forms, vector count + U grid strides, stays below 2^31
  S->wide = G.rows * G.nv + (int64_t)S->U * axes_grid(*S, G) * MD_BLOCK >= (1ll << 31) || md_opt(MD_OPT_JIT_AXES_WIDE) == 1;
}

}  // namespace jit
