// Shared device/host helpers for the xvit gfx950 kernels.  CDNA4 only: wave64, MFMA,
// buffer_load ... lds (LDS-DMA), ds_read_b64_tr_b16.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <mutex>
#include <type_traits>

#include "../../include/xvit.h"

namespace xvit {

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;

#define XVIT_LDS __attribute__((address_space(3)))

constexpr int kWave = 64;

// ---- error plumbing (host) -----------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);
const uint64_t* drop_epoch_ptr();   // xvit_set_dropout_epoch: device address of the dropout epoch counter, or nullptr (core.hip)
void set_attn_peel(int v);   // xvit_set_option("attn_peel") -> attention.hip

// One BLOCK-thread launch of KERNEL with LDS bytes of dynamic LDS.  More than the default 64 KiB has to be opted into per kernel:
// every launched instantiation does so at its first launch (a function-local static: thread-safe, the library is re-entrant).
template <auto KERNEL, int LDS, int BLOCK, class... Args>
static void launch_lds(dim3 grid, hipStream_t s, Args... args) {
  static const hipError_t opt_in = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  (void)opt_in;
  hipLaunchKernelGGL(KERNEL, grid, dim3(BLOCK), LDS, s, args...);
}

// The same for an LDS size known only at run time: the instantiation's limit is raised whenever a launch asks for more than the largest
// size seen so far (under a lock: the limit only ever grows, whichever threads launch).  Returns hipFuncSetAttribute's status; nothing
// is launched when it fails.
template <auto KERNEL, class... Args>
static hipError_t launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static std::mutex lock;
  static size_t limit = 64 * 1024;   // what a kernel may ask for without opting in
  {
    std::lock_guard<std::mutex> hold(lock);
    if (lds > limit) {
      const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      limit = lds;
    }
  }
  hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
  return hipSuccess;
}

// blocks of a grid-stride launch: one thread per unit of work, at most `cap` blocks
static inline int grid_for(int64_t work, int block, int cap = 4096) {
  const int64_t g = (work + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Run-time -> compile-time dispatch: f gets a value whose TYPE carries the choice (decltype(t), decltype(v)::value), so that a launch's
// argument list is written once for all its instantiations.
template <int V> using Int = std::integral_constant<int, V>;
template <class F>
static void by_dtype(int dtype, F&& f) {   // XVIT_F32 / XVIT_BF16 (host-checked)
  if (dtype == XVIT_F32) f(float{});
  else f(bf16{});
}
template <class F>
static void by_src_dtype(int dtype, F&& f) {   // by_dtype and XVIT_I16: the entry points that read raw volumes
  if (dtype == XVIT_I16) f(int16_t{});
  else by_dtype(dtype, f);
}
template <class F>
static void by_dtype_vec(int dtype, bool vec, F&& f) {   // by_dtype and Int<8> | Int<1>: elements per access, 8 where the caller found 16-byte runs
  by_dtype(dtype, [&](auto t) {
    if (vec) f(t, Int<8>{});
    else f(t, Int<1>{});
  });
}

static inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t all = 0;
  for (const void* p : ptrs) all |= reinterpret_cast<uintptr_t>(p);
  return (all & 15) == 0;
}

#define XVIT_REQUIRE(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      ::xvit::set_error(__VA_ARGS__);      \
      return XVIT_ERR_ARG;                 \
    }                                      \
  } while (0)

// What the draw entry points of the input stage (augment, elastic, contrast) refuse alike: under the caller's name, or as a predicate
// where the message is the caller's own.
#define XVIT_REQUIRE_COUNTER(who, counter, advance)                                                  \
  XVIT_REQUIRE(((uintptr_t)(counter) & 7) == 0, who ": the counter must be 8-byte aligned");         \
  XVIT_REQUIRE((counter) || !(advance), who ": advance needs a counter")
// What the entry points that take a [B, M, 1, D, H, W] volume and a patch refuse alike, under the caller's name (a const char*): reads the caller's B, M, D, H, W, dp, hp, wp, as every such entry point names them.
#define XVIT_REQUIRE_PATCH_GRID(who, dtypes_ok)                                                                                    \
  XVIT_REQUIRE(B > 0 && M > 0 && D > 0 && H > 0 && W > 0 && dp > 0 && hp > 0 && wp > 0, "%s: bad sizes", who);                    \
  XVIT_REQUIRE(D % dp == 0 && H % hp == 0 && W % wp == 0, "%s: image dimensions must be divisible by the patch size", who);       \
  XVIT_REQUIRE(dtypes_ok, "%s: bad dtype (bf16 or fp32)", who)
static inline bool dtype_ok(int dtype) { return dtype == XVIT_F32 || dtype == XVIT_BF16; }
static inline bool prob_ok(float p) { return p >= 0.f && p <= 1.f; }   // false for NaN
static inline bool range_ok(float lo, float hi) { return lo <= hi && isfinite(lo) && isfinite(hi); }

// ---- device helpers ------------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }  // v_cvt_pk_bf16_f32, RNE, NaN-safe

__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4& a) { return bf16x4{f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3])}; }
__device__ __forceinline__ bf16x8 to_bf16x8(const f32x4& a, const f32x4& b) {
  return bf16x8{f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(b[0]), f2bf(b[1]), f2bf(b[2]), f2bf(b[3])};
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Wave-uniform value made provably uniform for the compiler (SGPR).
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Buffer resource over [base, base+bytes): out-of-range loads return 0, stores are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

__device__ __forceinline__ uint32_t clamp_bytes(int64_t b) {
  return b <= 0 ? 0u : (b > 0x7FFFFFFFll ? 0x7FFFFFFFu : (uint32_t)b);
}

// 16-byte LDS-DMA: LDS[lds_base + lane*16 .. +16) <- buffer[voff + soff .. +16)
//
// Issued from inline asm on purpose.  With the __builtin_amdgcn_raw_ptr_buffer_load_lds form hipcc's
// waitcnt pass cannot prove that a later ds_read_b64_tr_b16 does not alias the DMA destination and puts
// `s_waitcnt vmcnt(0)` in front of the first transposed read of every iteration, which drains the
// next-stage prefetch before any MFMA has issued (seen in the NN/TN GEMM and all attention loops).  The
// kernels order DMA -> LDS read themselves (counted `s_waitcnt vmcnt` + s_barrier), so the compiler must
// simply not model these loads.  Untracked VMEM ops can only make the compiler's own vmcnt waits
// stricter, never weaker (the counter retires in order).  lds_base, soff and r must be wave-uniform.
// M0 is written in the same statement that consumes it; nothing else in these kernels uses M0.
#ifndef XVIT_GLDS_POLICY
#define XVIT_GLDS_POLICY ""      // cache-policy modifiers of the LDS-DMA loads (" nt", " sc1", ...): A/B builds only
#endif
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t r, XVIT_LDS void* lds_base, uint32_t voff, uint32_t soff) {
  const uint32_t m0v = (uint32_t)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen" XVIT_GLDS_POLICY " lds"
               :
               : "v"(voff), "s"(r), "s"(soff), "s"(m0v)
               : "memory");
}
// 4-byte variant: LDS[lds_base + lane*4 .. +4) <- buffer[voff + soff .. +4)
__device__ __forceinline__ void glds4(__amdgpu_buffer_rsrc_t r, XVIT_LDS void* lds_base, uint32_t voff, uint32_t soff) {
  const uint32_t m0v = (uint32_t)(uintptr_t)lds_base;
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %0, %1, %2 offen lds"
               :
               : "v"(voff), "s"(r), "s"(soff), "s"(m0v)
               : "memory");
}

__device__ __forceinline__ s16x4 lds_read_tr16(const XVIT_LDS void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((XVIT_LDS s16x4*)p);
}

// Wave-wide reductions, result in every lane.  Four DPP steps inside each 16-lane row (quad_perm, row_half_mirror, row_mirror: the
// operand permutation rides on the VALU instruction itself) and two row / half exchanges (v_permlane16_swap, v_permlane32_swap):
// eight VALU instructions, no LDS pipe.  (__shfl_xor compiles to ds_bpermute_b32: six dependent LDS round trips of ~100 cycles each,
// which is what a one-row-per-wave LayerNorm spends its time waiting on.)
template <int CTRL>
__device__ __forceinline__ float dpp_perm(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// v_permlane16_swap (W = 16) / v_permlane32_swap (W = 32) of x with itself: a = x of the even 16-lane row of each row pair (of the lower
// half of the wave), b = x of the odd row (upper half), in both.  ONE VALU instruction where __shfl_xor(x, W) is a ds_bpermute round trip.
// (Note for anyone touching this: __builtin_bit_cast(float, vec.y) on an ext-vector ELEMENT reads element 0 with this
// hipcc — go through a scalar temporary, as below.)
template <int W>
__device__ __forceinline__ void permlane_swap(float x, float& a, float& b) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t_;
  const unsigned bits = __builtin_bit_cast(unsigned, x);
  u32x2_t_ r;
  if constexpr (W == 16) r = __builtin_amdgcn_permlane16_swap(bits, bits, false, false);
  else r = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
  const unsigned r0 = r.x, r1 = r.y;
  a = __builtin_bit_cast(float, r0);
  b = __builtin_bit_cast(float, r1);
}
struct SumOp { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct MaxOp { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
template <class Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {
  v = op(v, dpp_perm<0xB1>(v));    // quad_perm [1, 0, 3, 2]
  v = op(v, dpp_perm<0x4E>(v));    // quad_perm [2, 3, 0, 1]
  v = op(v, dpp_perm<0x141>(v));   // row_half_mirror
  v = op(v, dpp_perm<0x140>(v));   // row_mirror
  float a, b;
  permlane_swap<16>(v, a, b);
  v = op(a, b);
  permlane_swap<32>(v, a, b);
  return op(a, b);
}
__device__ __forceinline__ float wave_sum(float v) { return wave_reduce(v, SumOp{}); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, MaxOp{}); }

// Block-wide reduction of an NW-wave block, result in every thread: each wave's result through red[NW], combined in wave order (fixed:
// bit-reproducible).  The leading barrier lets consecutive calls share `red`.
template <int NW, class Op>
__device__ __forceinline__ float block_reduce(float v, Op op, float* red) {
  v = wave_reduce(v, op);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = op(r, red[w]);
  return r;
}

// Combine a value across the two 32-lane halves of a wave (lane l with lane l ^ 32)
__device__ __forceinline__ float half_max(float x) {
  float lo, hi;
  permlane_swap<32>(x, lo, hi);
  return fmaxf(lo, hi);
}
__device__ __forceinline__ float half_sum(float x) {
  float lo, hi;
  permlane_swap<32>(x, lo, hi);
  return lo + hi;
}

// ---- shared by the attention kernels (attention.hip, attention_fp8.hip) ----------------
constexpr float LOG2E = 1.4426950408889634f;

// element index inside a 32-row accumulator block held in register i by lane half h
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// Workgroups are dealt to the 8 XCDs round-robin in dispatch order (x fastest), each XCD with its own L2.
// Remap the linear id so that a contiguous range of LOGICAL ids runs on one XCD: the query (or key) blocks of
// one (batch, head) then share an L2 and its K/V (Q/dO) tiles are fetched from HBM once, not once per XCD
// (measured before the remap: 350-390 MB fetched per launch against ~100 MB of q/k/v).
// The remap itself, bijective on [0, total): XCD x = lin % 8 gets the logical ids [x total / 8, (x + 1) total / 8), the first
// total % 8 XCDs one more.  What a kernel counts as `lin` and `total` decides which workgroups share an L2.
__device__ __forceinline__ int xcd_logical(int lin, int total) {
  const int q8 = total >> 3, r8 = total & 7, xcd = lin & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (lin >> 3);
}
struct BlockCoord { int x, head, b; };
__device__ __forceinline__ BlockCoord xcd_block_coord() {
  const int nx = gridDim.x, nh = gridDim.y;
  const int logical = xcd_logical(blockIdx.x + nx * (blockIdx.y + nh * blockIdx.z), nx * nh * gridDim.z);
  BlockCoord c;
  c.x = logical % nx;
  const int rest = logical / nx;
  c.head = rest % nh;
  c.b = rest / nh;
  return c;
}

// counted wait on the vector-memory counter (an LDS-DMA ring: "at most N loads still in flight")
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Exact-form (erf) GELU and its derivative in fp32.  erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7,
// i.e. fp32 round-off level; libm erff costs ~4x the VALU work and the epilogue is VALU-bound):
//   erf(u) = 1 - (a1 t + a2 t^2 + a3 t^3 + a4 t^4 + a5 t^5) e^{-u^2},  t = 1 / (1 + p u),  u >= 0.
// GELU and GELU' share the one exponential: with u = |x|/sqrt(2), e^{-u^2} = e^{-x^2/2} is also the
// normal pdf up to 1/sqrt(2 pi).
__device__ __forceinline__ void gelu_parts(float x, float& cdf, float& pdf) {
  const float u = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, u, 1.0f));
  const float e = __expf(-u * u);
  float poly = fmaf(1.061405429f, t, -1.453152027f);
  poly = fmaf(poly, t, 1.421413741f);
  poly = fmaf(poly, t, -0.284496736f);
  poly = fmaf(poly, t, 0.254829592f);
  const float erf_abs = fmaf(-poly * t, e, 1.0f);
  cdf = 0.5f * (1.0f + copysignf(erf_abs, x));
  pdf = 0.39894228040143268f * e;
}
__device__ __forceinline__ float gelu_f(float x) {
  float cdf, pdf;
  gelu_parts(x, cdf, pdf);
  return x * cdf;
}
__device__ __forceinline__ void gelu_and_grad(float x, float& a, float& d) {   // a = gelu(x), d = gelu'(x): one exponential for both
  float cdf, pdf;
  gelu_parts(x, cdf, pdf);
  a = x * cdf;
  d = fmaf(x, pdf, cdf);
}
__device__ __forceinline__ float dgelu_f(float x) {
  float cdf, pdf;
  gelu_parts(x, cdf, pdf);
  return fmaf(x, pdf, cdf);
}

// counter-based RNG for dropout: one 32-bit hash per element index (same mask in fwd and bwd)
__device__ __forceinline__ uint32_t hash32(uint64_t seed, uint64_t idx) {
  uint64_t z = idx * 0x9E3779B97F4A7C15ull + seed;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

__device__ __forceinline__ uint32_t draw24(uint64_t seed, uint64_t idx) { return hash32(seed, idx) & 0xFFFFFFu; }   // uniform on [0, 2^24)
constexpr float kTwo24 = 16777216.0f, kInv24 = 1.0f / kTwo24;
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t idx) { return (float)draw24(seed, idx) * kInv24; }   // [0, 1), exact
__device__ __forceinline__ float uniform_in(uint64_t seed, uint64_t idx, float lo, float hi) {                          // [lo, hi], clamped
  return fminf(fmaxf(fmaf(uniform01(seed, idx), hi - lo, lo), lo), hi);
}

// A captured step (HIP graph) freezes every kernel argument, the dropout seeds included.  A launch may therefore carry the device address
// of an epoch counter (xvit_set_dropout_epoch): the seed a kernel then uses is seed + epoch * odd constant, read at run time, so that a
// replay whose graph increments the counter first draws new masks — the same ones in its forward and its backward.
constexpr uint64_t kSeedStride = 0xD1B54A32D192ED03ull;
__device__ __forceinline__ uint64_t drop_seed_at(uint64_t seed, const uint64_t* __restrict__ epoch) {
  return epoch ? seed + *epoch * kSeedStride : seed;
}
// The draw kernels of the input stage step their seed the same way by the call index `count` they read from their counter (0 without
// one), and xor the salt that keeps their stream apart from the other stages' under one seed.
__device__ __forceinline__ uint64_t draw_seed(uint64_t seed, uint64_t count, uint64_t salt) { return (seed + count * kSeedStride) ^ salt; }

// Dropout at rate p as a launch carries it.  Element idx is kept iff its 24-bit draw >= p 2^24 and then scaled by inv = 1 / (1 - p): the
// mask of xvit_dropout on a contiguous tensor with this seed, regenerated wherever it is needed (forward and backward), never stored.
// p 2^24 is exact in fp32, on the host as on the device.
struct Dropout {
  float p = 0.f, inv = 1.f;
  uint32_t thr = 0;
  uint64_t seed = 0;
  const uint64_t* epoch = nullptr;   // drop_seed_at (captured steps), or nullptr
  Dropout() = default;
  Dropout(float p_, uint64_t seed_) : p(p_), inv(1.0f / (1.0f - p_)), thr((uint32_t)(p_ * kTwo24)), seed(seed_), epoch(p_ > 0.f ? drop_epoch_ptr() : nullptr) {}   // host
  __device__ __forceinline__ bool on() const { return p > 0.f; }
  __device__ __forceinline__ Dropout at_run_time() const {   // once per thread: the seed of this launch (or replay)
    Dropout d = *this;
    d.seed = drop_seed_at(seed, epoch);
    return d;
  }
  __device__ __forceinline__ bool keep(uint64_t idx) const { return draw24(seed, idx) >= thr; }
};

}  // namespace xvit
