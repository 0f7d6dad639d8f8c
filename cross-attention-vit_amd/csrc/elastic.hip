// Elastic deformation (include/xvit.h, "Elastic deformation"): xvit_elastic_draw fills one cubic B-spline control grid per SAMPLE from a
// config and a seed; xvit_augment_apply_elastic is xvit_augment_apply with the grid's displacement composed into its one resample,
// p = A (q + u(q)) + t, computed as p_affine + A u.  A sample whose flag is 0 runs the code of augment_apply_kernel itself (augment_apply.h)
// and its field is never read.
//
// The B-spline sums, in the fixed order that makes two runs bit-identical (no atomics, nothing depends on the execution order):
//   weights    B0 = (1 - t)^3 k, B1 = fmaf(t t, fmaf(3, t, -6), 4) k, B2 = fmaf(t, fmaf(t, fmaf(-3, t, 3), 3), 1) k, B3 = t^3 k, k = fl(1 / 6)
//   rows       R_k[gx] = sum over a = 0..3 (z, outer), b = 0..3 (y, inner) of fmaf(Bz_a By_b, phi_k[cz + a, cy + b, gx], acc), acc from 0
//   voxel      u_k = fmaf(Bx_3, R_k[cx + 3], fmaf(Bx_2, R_k[cx + 2], fmaf(Bx_1, R_k[cx + 1], Bx_0 R_k[cx])))
//   compose    p_i = p_affine_i + fmaf(A_i2, u_x, fmaf(A_i1, u_y, A_i0 u_z))
// A zero field gives u = 0 and A u = 0 exactly: the result is that of xvit_augment_apply's general path, bit for bit.
//
// Where the control points are read.  The B-spline is separable and the z and y weights of a destination row are shared by every lane on
// it, so a workgroup reduces the 4 x 4 (z, y) control rows ONCE PER DESTINATION ROW of its brick (256 >> lx rows, not once per lane) into
// the x-coefficients R_k[0 .. Gx - 1] and keeps them in LDS (at most 64 rows x 49 floats = 12.5 KB; the row stride of 49 keeps the rows
// of a wave on different banks).  LDS was chosen over scalar / L1 reads because the reduction is shared by the 4 to 16 lanes of a row: it
// costs 16 L1-resident loads per coefficient, 3 Gx coefficients per row, spread over the 256 threads (about 21 loads a thread for a 7^3
// grid on a 128 x 4 x 4 brick, against 240 a lane if every lane reduced for itself), and one barrier.  Behind the barrier a lane reads
// five coefficients per component when the x cell changes at most once inside its 8 voxels (any grid with W >= 8 (Gx - 3)), and then
// spends 4 multiply-adds per component and voxel; a run that crosses more cells reads its four coefficients per voxel.  The 8 x 3
// displacements are formed first, in either way, and one loop of trilinear taps follows: the large part of the code exists once.
#include <math.h>

#include "augment_apply.h"

namespace xvit {

constexpr uint64_t kElaSalt = 0x00454C4153544943ull;     // "ELASTIC": keeps this stream apart from the augment and contrast streams under one seed
constexpr int kElaSampleStride = 16384, kElaPointBase = 16;   // hash indices per sample; the first control point's index
constexpr int kElaRowStride = 3 * XVIT_ELASTIC_MAX_GRID + 1;  // floats per destination row in LDS

struct ElasticGeom {
  int Gz, Gy, Gx;
  float sz, sy, sx;   // (G - 3) / (n - 1) in fp32, rounded once on the host; 0 when n = 1
};

// ------------------------------------------------------------------------------------------
// draw: one block per sample.  Every block reads the counter; a launch of its own advances it afterwards (elastic_advance_kernel), so
// that no block can see the advanced value.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) elastic_draw_kernel(xvit_elastic_config c, float* __restrict__ field, float* __restrict__ erec, int Gz, int Gy, int Gx,
                                                           uint64_t seed, const uint64_t* counter) {
  __shared__ float red[3][256];
  const uint64_t count = counter ? *counter : 0;
  const uint64_t s = draw_seed(seed, count, kElaSalt);
  const int b = blockIdx.x, L = c.locked_borders;
  const uint64_t i0 = (uint64_t)kElaSampleStride * (uint64_t)b;
  const float udec = uniform01(s, i0);
  const bool active = udec < c.prob;

  const int per = Gz * Gy * Gx;
  float* __restrict__ F = field + (int64_t)b * 3 * per;
  float mx[3] = {0.f, 0.f, 0.f};
  for (int idx = threadIdx.x; idx < 3 * per; idx += 256) {
    const int a = idx / per;
    int rem = idx - a * per;
    const int gx = rem % Gx;
    rem /= Gx;
    const int gy = rem % Gy, gz = rem / Gy;
    const bool locked = gz < L || gz >= Gz - L || gy < L || gy >= Gy - L || gx < L || gx >= Gx - L;
    float v = 0.f;
    if (active && !locked) {
      const float m = c.max_displacement[a];
      v = uniform_in(s, i0 + kElaPointBase + idx, -m, m);   // m - -m = 2 m exactly
    }
    F[idx] = v;
    for (int k = 0; k < 3; ++k) mx[k] = a == k ? fmaxf(mx[k], fabsf(v)) : mx[k];
  }
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = mx[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = fmaxf(red[k][threadIdx.x], red[k][threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x < XVIT_ELASTIC_NREC) {
    const int k = threadIdx.x;
    erec[(int64_t)b * XVIT_ELASTIC_NREC + k] = k == 0 ? (active ? 1.f : 0.f) : k == 1 ? udec : k <= 4 ? red[k - 2][0] : 0.f;
  }
}

__global__ void elastic_advance_kernel(uint64_t* counter) { *counter += 1; }

// ------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------
// the cell and the four cubic B-spline weights of destination index i along an axis: g = i s, c = min(floor(g), G - 4), t = g - c
__device__ __forceinline__ int bspline_cell(int i, float s, int G, float (&B)[4]) {
  const float g = (float)i * s;
  const int c = min((int)floorf(g), G - 4);
  const float t = g - (float)c, omt = 1.f - t;
  constexpr float k = 1.f / 6.f;
  B[0] = omt * omt * omt * k;
  B[1] = fmaf(t * t, fmaf(3.f, t, -6.f), 4.f) * k;
  B[2] = fmaf(t, fmaf(t, fmaf(-3.f, t, 3.f), 3.f), 1.f) * k;
  B[3] = t * t * t * k;
  return c;
}

template <typename S, typename T>
__global__ void __launch_bounds__(256) augment_apply_elastic_kernel(const S* __restrict__ src, T* __restrict__ dst, const float* __restrict__ params,
                                                                    const float* __restrict__ field, const float* __restrict__ erec, int M, AugGeom g,
                                                                    ElasticGeom e, int lx, int nbx, int nby, int nbz, float pad_value) {
  __shared__ float coef[64 * kElaRowStride];
  const AugLane L = aug_locate(g, lx, nbx, nby, nbz);
  // The record and the flag are workgroup-uniform scalar loads.  The whole record is copied here, in front of the branch on the flag, so
  // that both loads are in flight together: read behind the branch, the record would wait for the flag's round trip first.
  const float* __restrict__ Pg = params + (int64_t)L.vol * XVIT_AUG_NPARAM;
  const int sample = L.vol / M;
  const float flag = erec[(int64_t)sample * XVIT_ELASTIC_NREC];
  float P[XVIT_AUG_NPARAM];
#pragma unroll
  for (int k = 0; k < XVIT_AUG_NPARAM; ++k) P[k] = Pg[k];
  if (flag == 0.f) {   // the field is not read, no barrier is met
    if (L.inside) aug_apply_lane(src, dst, P, g, L, pad_value);
    return;
  }

  // every destination row (z, y) of the brick: its 4 x 4 control rows reduced into R_k[0 .. Gx - 1], k = z, y, x
  const int ny = 64 >> lx, per_row = 3 * e.Gx, total = (256 >> lx) * per_row;
  const float* __restrict__ F = field + (int64_t)sample * 3 * e.Gz * e.Gy * e.Gx;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int r = idx / per_row, rem = idx - r * per_row;
    const int k = rem / e.Gx, gx = rem - k * e.Gx;
    const int z = L.bz * 4 + r / ny, y = L.by * ny + r % ny;   // row r belongs to wave r / ny, lanes with lane >> lx == r % ny
    if (z >= g.D || y >= g.H) continue;
    float Bz[4], By[4];
    const int cz = bspline_cell(z, e.sz, e.Gz, Bz), cy = bspline_cell(y, e.sy, e.Gy, By);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc = fmaf(Bz[a] * By[b], F[((k * e.Gz + cz + a) * e.Gy + cy + b) * e.Gx + gx], acc);   // indices <= G - 1 by the min in bspline_cell
    coef[r * kElaRowStride + k * XVIT_ELASTIC_MAX_GRID + gx] = acc;
  }
  __syncthreads();
  if (!L.inside) return;

  const int row = (int)(threadIdx.x >> 6) * ny + (int)((threadIdx.x & 63) >> lx);
  const float* __restrict__ R = coef + row * kElaRowStride;
  float Bx[4];
  const int c_first = bspline_cell(L.x0, e.sx, e.Gx, Bx), c_last = bspline_cell(L.x0 + L.n - 1, e.sx, e.Gx, Bx);
  const bool one_step = c_last - c_first <= 1;   // the cell changes at most once inside the run: five coefficients serve it
  // the displacement of the run's 8 voxels (those behind the run's end are computed and not stored, as in aug_general_run); both
  // branches feed the same four coefficients into the same sum, so they give the same bits
  float u[8][3];
  if (one_step) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* __restrict__ Rk = R + k * XVIT_ELASTIC_MAX_GRID;
      const float r0 = Rk[c_first], r1 = Rk[c_first + 1], r2 = Rk[c_first + 2], r3 = Rk[c_first + 3], r4 = Rk[min(c_first + 4, e.Gx - 1)];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool up = bspline_cell(L.x0 + i, e.sx, e.Gx, Bx) > c_first;
        u[i][k] = fmaf(Bx[3], up ? r4 : r3, fmaf(Bx[2], up ? r3 : r2, fmaf(Bx[1], up ? r2 : r1, Bx[0] * (up ? r1 : r0))));
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float* __restrict__ Rc = R + bspline_cell(L.x0 + i, e.sx, e.Gx, Bx);   // cell + 3 <= Gx - 1
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* __restrict__ Rk = Rc + k * XVIT_ELASTIC_MAX_GRID;
        u[i][k] = fmaf(Bx[3], Rk[3], fmaf(Bx[2], Rk[2], fmaf(Bx[1], Rk[1], Bx[0] * Rk[0])));
      }
    }
  }

  const int flags = (int)P[XVIT_AUG_FLAGS];
  const S* __restrict__ sv = src + (int64_t)L.vol * g.Ds * g.Hs * g.Ws;
  const AugAffine aff(P, L);
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float pz, py, px;
    aff.at((float)(L.x0 + i), pz, py, px);
    pz += fmaf(P[2], u[i][2], fmaf(P[1], u[i][1], P[0] * u[i][0]));
    py += fmaf(P[6], u[i][2], fmaf(P[5], u[i][1], P[4] * u[i][0]));
    px += fmaf(P[10], u[i][2], fmaf(P[9], u[i][1], P[8] * u[i][0]));
    v[i] = aug_trilinear(sv, g, pz, py, px, pad_value);
  }
  aug_finish_run(P, flags, g, L, dst, v);
}

static bool grid_ok(int G) { return G >= 4 && G <= XVIT_ELASTIC_MAX_GRID; }
static float grid_step(int G, int n) { return n > 1 ? (float)(G - 3) / (float)(n - 1) : 0.f; }

// What both entry points refuse about the grid and its buffers, under the caller's name.
#define XVIT_ELASTIC_REQUIRE_GRID(who)                                                                                                                      \
  XVIT_REQUIRE(xvit::grid_ok(Gz) && xvit::grid_ok(Gy) && xvit::grid_ok(Gx), who ": grid %d x %d x %d: every axis needs 4 .. %d control points", Gz, Gy, Gx, \
               XVIT_ELASTIC_MAX_GRID)
#define XVIT_ELASTIC_REQUIRE_ALIGNED(who) \
  XVIT_REQUIRE(((uintptr_t)field & 15) == 0 && ((uintptr_t)erec & 15) == 0, who ": the field and the record must be 16-byte aligned")

}  // namespace xvit

extern "C" int xvit_elastic_draw(const xvit_elastic_config* config, float* field, float* erec, int B, int Gz, int Gy, int Gx, uint64_t seed, uint64_t* counter,
                                 int advance, xvit_stream_t stream) {
  XVIT_REQUIRE(config && field && erec, "xvit_elastic_draw: null config, field or record");
  XVIT_REQUIRE(B > 0 && B < (1 << 17), "xvit_elastic_draw: B=%d must be positive and below 2^17", B);
  XVIT_ELASTIC_REQUIRE_GRID("xvit_elastic_draw");
  const xvit_elastic_config& c = *config;
  XVIT_REQUIRE(xvit::prob_ok(c.prob), "xvit_elastic_draw: the probability must lie in [0, 1]");
  for (int k = 0; k < 3; ++k)
    XVIT_REQUIRE(c.max_displacement[k] >= 0.f && isfinite(c.max_displacement[k]), "xvit_elastic_draw: max_displacement[%d]=%g must be finite and >= 0", k,
                 c.max_displacement[k]);
  XVIT_REQUIRE(c.locked_borders >= 0 && c.locked_borders <= 3, "xvit_elastic_draw: locked_borders=%d must lie in 0 .. 3", c.locked_borders);
  XVIT_ELASTIC_REQUIRE_ALIGNED("xvit_elastic_draw");
  XVIT_REQUIRE_COUNTER("xvit_elastic_draw", counter, advance);
  hipLaunchKernelGGL(xvit::elastic_draw_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, c, field, erec, Gz, Gy, Gx, seed, counter);
  if (advance) hipLaunchKernelGGL(xvit::elastic_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter);
  return xvit::check_launch("xvit_elastic_draw");
}

extern "C" int xvit_augment_apply_elastic(const void* src, int src_dtype, void* dst, int dst_dtype, const float* params, const float* field, const float* erec,
                                          int nvol, int M, int Gz, int Gy, int Gx, int Ds, int Hs, int Ws, int D, int H, int W, float pad_value,
                                          xvit_stream_t stream) {
  XVIT_AUG_APPLY_REQUIRE("xvit_augment_apply_elastic");
  XVIT_REQUIRE(M > 0 && nvol % M == 0, "xvit_augment_apply_elastic: nvol=%d is no multiple of M=%d", nvol, M);
  XVIT_ELASTIC_REQUIRE_GRID("xvit_augment_apply_elastic");
  XVIT_REQUIRE(field && erec, "xvit_augment_apply_elastic: null field or record");
  XVIT_ELASTIC_REQUIRE_ALIGNED("xvit_augment_apply_elastic");
  const xvit::AugGeom g = xvit::make_geom(Ds, Hs, Ws, D, H, W);
  const xvit::ElasticGeom e{Gz, Gy, Gx, xvit::grid_step(Gz, D), xvit::grid_step(Gy, H), xvit::grid_step(Gx, W)};
  const xvit::AugBricks b(g);
  xvit::by_src_dtype(src_dtype, [&](auto sd) {
    xvit::by_dtype(dst_dtype, [&](auto dd) {
      using S = decltype(sd);
      using T = decltype(dd);
      hipLaunchKernelGGL((xvit::augment_apply_elastic_kernel<S, T>), dim3(b.blocks(nvol)), dim3(256), 0, (hipStream_t)stream, (const S*)src, (T*)dst, params,
                         field, erec, M, g, e, b.lx, b.nbx, b.nby, b.nbz, pad_value);
    });
  });
  return xvit::check_launch("xvit_augment_apply_elastic");
}
