// Wide Krylov bases for the block eigensolver (curvlinops_amd/eigensolver.py): float32 Q [D][ldq] with 1 <= m <= 1024
// columns against narrow blocks W [D][ldw] with 1 <= b <= 64 columns, 64-bit row indexing, any leading dimension.
//
//   clo_basis_project_f64   C [m][b] (float64) = Q^T W.  Q is streamed once: a block owns one 64-column tile of Q
//                           (grid.y) and a set of 64-row chunks (grid.x); [Q tile | W] rows are staged in LDS with
//                           16-byte loads (the next chunk's loads in flight while the current one is multiplied) and
//                           contracted over the rows on v_mfma_f64_16x16x4_f64: EXACT products (24 x 24-bit), float64
//                           accumulation.  W is read once per 64-column tile of Q.
//                           bytes = 4 D (m + ceil(m / 64) b);  flops = 2 D 64 ceil(m / 64) 16 ceil(b / 16).
//   clo_basis_update_f32    W <- W - Q C (C float64 [m][b], rounded to float32 once), and with a non-NULL C2 in the same
//                           pass C2 [m][b] (float64) = Q^T W_new.  A block owns 16 columns of W (grid.y) and walks chunks
//                           of 16 rows: the chunk's Q rows [16][m] are staged in LDS (swizzled, conflict-free for both
//                           access patterns), the four waves split the contraction over m (float32 MFMA 16x16x4, C in
//                           registers), the partial 16 x 16 tiles are summed in a fixed order, W_new is written back and
//                           kept in LDS, and the waves then contract Q^T W_new over the chunk's rows on the f64 MFMA
//                           (exact products).  Each row of W_new depends only on its own row of Q, so both products share
//                           one read of Q:  bytes = 4 D (ceil(b / 16) m + 2 b).  CGS2 thus costs three reads of Q:
//                           project, update + reproject, update.
//   clo_basis_combine_f32   Y [D][p] = Q S (S float64 [m][p], 1 <= p <= 1024) out of place: the update kernel without
//                           the input block and the reprojection; bytes = 4 D (ceil(p / 16) m + p).  It runs once per
//                           restart (p = the kept Ritz vectors), never per block step.
//   clo_basis_ws_bytes      workspace of project / update: per-block float64 partials, reduced by a second launch in a
//                           fixed order (bit-identical on repeat).
//
// D = 0 computes empty sums (C = 0, C2 = 0) and touches no row.  Nothing here synchronises the device.
#include "clo_common.h"

namespace clo {
namespace {

using f64x4b = __attribute__((ext_vector_type(4))) double;
using f32x4b = __attribute__((ext_vector_type(4))) float;

constexpr int BS_THREADS = 256;
constexpr int BS_MAX_M = 1024, BS_MAX_B = 64, BS_MAX_P = 1024;

// ------------------------------------------------------------------------------------------------------------ project
constexpr int PJ_RC = 64;   // rows per staged chunk (16 per wave = four K-steps of the f64 MFMA)

struct ProjArgs {
  const float *Q, *W;
  long ldq, ldw, D;
  int m, b, vecq, vecw, gx;
  double *slab;   // [ceil(m / 64)][gx][64][16 NJ]
};

template <int NJ>
__global__ __launch_bounds__(BS_THREADS) void basis_project_kernel(const ProjArgs p) {
  constexpr int P1 = 64, P2 = 16 * NJ, PT = P1 + P2;
  constexpr int PITCH = ((PT + 15) / 32) * 32 + 16;   // = 16 mod 32: the four rows of one ds_read_b32 hit disjoint banks
  constexpr int QPR = PT / 4;                         // 16-byte pieces per staged row
  constexpr int NLD = (PJ_RC * QPR + BS_THREADS - 1) / BS_THREADS;
  __shared__ __attribute__((aligned(16))) float St[PJ_RC * PITCH];
  __shared__ double S[4 * 256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, r = lane >> 4;
  const int c0 = blockIdx.y * 64;
  const int nq = min(64, p.m - c0), nw = p.b;
  f64x4b acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f64x4b{0., 0., 0., 0.};
  int prow[NLD], pcol[NLD];
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    const int e = min(tid + u * BS_THREADS, PJ_RC * QPR - 1);
    prow[u] = e / QPR;
    pcol[u] = (e - prow[u] * QPR) * 4;
  }
  // staged columns [0, 64) come from the Q tile, [64, PT) from W; rows >= D and columns past the operand are zero
  auto fetch = [&](long r0, float4 (&v)[NLD]) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const long row = r0 + prow[u];
      const int sc = pcol[u];
      const bool fromq = sc < P1;
      const int col = fromq ? sc : sc - P1;
      const int nn = fromq ? nq : nw;
      float t[4] = {0.f, 0.f, 0.f, 0.f};
      if (row < p.D && col < nn) {
        const float *base = fromq ? p.Q + row * p.ldq + c0 + col : p.W + row * p.ldw + col;
        if (fromq ? p.vecq : p.vecw) {   // (vec: the operand's width is a multiple of 4, col + 3 < nn)
          const float4 x = *reinterpret_cast<const float4 *>(base);
          t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[e] = col + e < nn ? base[e] : 0.f;
        }
      }
      v[u] = make_float4(t[0], t[1], t[2], t[3]);
    }
  };
  const long nchunks = cdiv(p.D, (long)PJ_RC);
  float4 cur[NLD];
  if ((long)blockIdx.x < nchunks) fetch((long)blockIdx.x * PJ_RC, cur);
  for (long ch = blockIdx.x; ch < nchunks; ch += p.gx) {
    __syncthreads();   // everybody is done with the previous chunk
#pragma unroll
    for (int u = 0; u < NLD; ++u)
      if (tid + u * BS_THREADS < PJ_RC * QPR) *reinterpret_cast<float4 *>(&St[prow[u] * PITCH + pcol[u]]) = cur[u];
    fetch((ch + p.gx) * PJ_RC, cur);   // (past the end: zeros, no loads)
    __syncthreads();
    const float *sp = St + (wave * (PJ_RC / 4) + r) * PITCH + c;
#pragma unroll
    for (int st = 0; st < PJ_RC / 16; ++st) {
      double a[4], bb[NJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = (double)sp[st * 4 * PITCH + 16 * i];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bb[j] = (double)sp[st * 4 * PITCH + P1 + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
  }
  // the four waves' tiles are summed through LDS in a fixed order (f64 16x16x4 D layout: row = lane / 16 + 4 q,
  // col = lane % 16); every block writes its whole partial, zeros included
  __syncthreads();
  double *out = p.slab + ((long)blockIdx.y * p.gx + blockIdx.x) * 64 * P2;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) S[wave * 256 + (r + 4 * q) * 16 + c] = acc[i][j][q];
      __syncthreads();
      {
        const int e = tid, row = e >> 4, col = e & 15;
        out[(long)(16 * i + row) * P2 + 16 * j + col] = (S[e] + S[256 + e]) + (S[512 + e] + S[768 + e]);
      }
      __syncthreads();
    }
}

// out[a][col0 + jj] = sum over bx of slab[((T gx + bx) R + rr) P + jj], jj < P; T / rr: the 64-row tile of a and the row
// in it (project, row_tiled) or grid.y and a (update).  256 / P lanes per column sum strided block partials, then the
// lanes are added in order: fixed order, bit-identical on repeat.
__global__ __launch_bounds__(BS_THREADS) void basis_reduce_kernel(double *__restrict__ out, long ldo,
                                                                  const double *__restrict__ slab, int gx, int R, int P,
                                                                  int ncols, int row_tiled) {
  __shared__ double red[BS_THREADS];
  const int a = blockIdx.x, ty = blockIdx.y;
  const int T = row_tiled ? a / R : ty, rr = row_tiled ? a % R : a, col0 = row_tiled ? 0 : 16 * ty;
  const int lanes = BS_THREADS / P;
  const int jj = threadIdx.x % P, s = threadIdx.x / P;
  double acc = 0.;
  if (s < lanes)
    for (int bx = s; bx < gx; bx += lanes) acc += slab[(((long)T * gx + bx) * R + rr) * P + jj];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (s == 0 && col0 + jj < ncols) {
    double t = 0.;
    for (int q = 0; q < lanes; ++q) t += red[q * P + jj];
    out[(long)a * ldo + col0 + jj] = t;
  }
}

inline int project_gx(long D, int m) {
  const int nty = (int)cdiv(m, 64);
  return (int)std::max<long>(1, std::min<long>(cdiv(D, (long)PJ_RC), std::max(1, 4 * kNumCU / nty)));
}

// ------------------------------------------------------------------------------------------------------ update / combine
// MT: 16-column tiles of Q per wave (the waves own consecutive quarters of the 64 MT columns staged).  The chunk is stored
// k-major, Qs[k][16] with the row index XOR-ed by 4 ((k >> 2) & 3): the update's A operand (row i, column c + 4 e + g)
// and the reprojection's A operand (column c + i, row 4 kk + g) both hit 64 distinct banks.
struct UpdArgs {
  float *out;
  const float *W, *Q;
  const double *C;
  double *slab;   // [grid.y][gx][m][16], or NULL
  long ldo, ldw, ldq, ldc, D;
  int m, n, vecq, gx;
  float alpha;
};

__device__ __forceinline__ int qs_index(int k, int r) { return k * 16 + (r ^ (((k >> 2) & 3) << 2)); }

template <int MT>
__global__ __launch_bounds__(BS_THREADS) void basis_update_kernel(const UpdArgs p) {
  constexpr int MQ = 64 * MT;            // staged columns
  constexpr int QPR = MQ / 4;            // 16-byte pieces per row of the chunk
  constexpr int NLD = 16 * QPR / BS_THREADS;   // = MT
  __shared__ __attribute__((aligned(16))) float Qs[MQ * 16];
  __shared__ float Ps[4 * 256];
  __shared__ float Wn[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int j0 = 16 * blockIdx.y;
  const bool reproj = p.slab != nullptr;
  // this lane's coefficients: C[c + 4 e + g][j0 + i] for the wave's tiles c = 16 (MT wave + kt)
  float cb[MT][4];
#pragma unroll
  for (int kt = 0; kt < MT; ++kt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 16 * (MT * wave + kt) + 4 * e + g, col = j0 + i;
      cb[kt][e] = (k < p.m && col < p.n) ? (float)p.C[(long)k * p.ldc + col] : 0.f;
    }
  f64x4b acc2[MT];
#pragma unroll
  for (int kt = 0; kt < MT; ++kt) acc2[kt] = f64x4b{0., 0., 0., 0.};
  // thread's pieces of a chunk: (row, 4-column group); its element of the 16 x 16 output tile: (erow, ecol)
  const int erow = tid >> 4, ecol = tid & 15;
  auto fetch = [&](long r0, float4 (&v)[NLD], float &w) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + u * BS_THREADS, rr = e / QPR, col = (e - rr * QPR) * 4;
      const long row = r0 + rr;
      float t[4] = {0.f, 0.f, 0.f, 0.f};
      if (row < p.D && col < p.m) {
        const float *base = p.Q + row * p.ldq + col;
        if (p.vecq) {   // (vec: m % 4 == 0, so col + 3 < m)
          const float4 x = *reinterpret_cast<const float4 *>(base);
          t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) t[q] = col + q < p.m ? base[q] : 0.f;
        }
      }
      v[u] = make_float4(t[0], t[1], t[2], t[3]);
    }
    const long row = r0 + erow;
    w = (p.W && row < p.D && j0 + ecol < p.n) ? p.W[row * p.ldw + j0 + ecol] : 0.f;
  };
  const long nchunks = cdiv(p.D, 16L);
  float4 cur[NLD];
  float wcur = 0.f;
  if ((long)blockIdx.x < nchunks) fetch((long)blockIdx.x * 16, cur, wcur);
  for (long ch = blockIdx.x; ch < nchunks; ch += p.gx) {
    const long r0 = ch * 16;
    __syncthreads();   // everybody is done with the previous chunk
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + u * BS_THREADS, rr = e / QPR, col = (e - rr * QPR) * 4;
      Qs[qs_index(col, rr)] = cur[u].x;
      Qs[qs_index(col + 1, rr)] = cur[u].y;
      Qs[qs_index(col + 2, rr)] = cur[u].z;
      Qs[qs_index(col + 3, rr)] = cur[u].w;
    }
    const float w_in = wcur;
    fetch(r0 + 16L * p.gx, cur, wcur);   // (past the end: zeros, no loads)
    __syncthreads();
    // ---- this wave's share of (Q C)[16 rows][16 columns]: f32 16x16x4, A = Q[row i][k], B = C[k][col i], k = c + 4 e + g
    f32x4b acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < MT; ++kt) {
      const int c = 16 * (MT * wave + kt);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[qs_index(c + 4 * e + g, i)], cb[kt][e], acc, 0, 0, 0);
    }
    // f32 16x16x4 D layout: row = 4 (lane / 16) + q, col = lane % 16
#pragma unroll
    for (int q = 0; q < 4; ++q) Ps[wave * 256 + (4 * g + q) * 16 + i] = acc[q];
    __syncthreads();
    {
      const float v = (Ps[tid] + Ps[256 + tid]) + (Ps[512 + tid] + Ps[768 + tid]);
      const long row = r0 + erow;
      const int col = j0 + ecol;
      float wn = 0.f;
      if (row < p.D && col < p.n) {
        wn = fmaf(p.alpha, v, w_in);
        p.out[row * p.ldo + col] = wn;
      }
      Wn[tid] = wn;
    }
    if (reproj) {
      __syncthreads();
      // ---- C2[c + i][col] += sum over the chunk's rows: f64 16x16x4, A = Q[row 4 kk + g][column c + i], B = W_new[row][i]
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double bw = (double)Wn[(4 * kk + g) * 16 + i];
#pragma unroll
        for (int kt = 0; kt < MT; ++kt) {
          const int c = 16 * (MT * wave + kt);
          acc2[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)Qs[qs_index(c + i, 4 * kk + g)], bw, acc2[kt], 0, 0, 0);
        }
      }
    }
  }
  if (reproj) {
    // the block's partial C2 for its 16 columns (f64 16x16x4 D layout: row = lane / 16 + 4 q, col = lane % 16)
    double *out = p.slab + ((long)blockIdx.y * p.gx + blockIdx.x) * p.m * 16;
#pragma unroll
    for (int kt = 0; kt < MT; ++kt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 16 * (MT * wave + kt) + g + 4 * q;
        if (k < p.m) out[(long)k * 16 + i] = acc2[kt][q];
      }
  }
}

inline int update_mt(int m) {
  const int t = (int)cdiv(m, 64);
  return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : 16;
}

// blocks per CU over all 16-column tiles: enough co-resident waves to hide the chunk loads (the staged chunk is 4 MT KiB)
// (MT >= 8 compiles to 1 wave per SIMD: one 4-wave block per CU)
inline int update_per_cu(int mt) { return mt == 1 ? 8 : mt == 2 ? 4 : mt == 4 ? 2 : 1; }
inline int update_gx(long D, int m, int n) {
  const int nty = (int)cdiv(n, 16);
  return (int)std::max<long>(1, std::min<long>(cdiv(D, 16L), std::max(1, update_per_cu(update_mt(m)) * kNumCU / nty)));
}

int launch_update(const UpdArgs &a, hipStream_t st) {
  const dim3 grid(a.gx, (unsigned)cdiv(a.n, 16));
  switch (update_mt(a.m)) {
    case 1: hipLaunchKernelGGL(basis_update_kernel<1>, grid, dim3(BS_THREADS), 0, st, a); break;
    case 2: hipLaunchKernelGGL(basis_update_kernel<2>, grid, dim3(BS_THREADS), 0, st, a); break;
    case 4: hipLaunchKernelGGL(basis_update_kernel<4>, grid, dim3(BS_THREADS), 0, st, a); break;
    case 8: hipLaunchKernelGGL(basis_update_kernel<8>, grid, dim3(BS_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL(basis_update_kernel<16>, grid, dim3(BS_THREADS), 0, st, a); break;
  }
  CLO_CHECK_LAUNCH("basis_update_kernel");
  return CLO_OK;
}

}  // namespace
}  // namespace clo

using namespace clo;

// An upper bound over every call with m' <= m and b' <= b (the grids shrink as m' grows, so a workspace sized for the
// widest basis alone would be too small for a narrower one): project writes ceil(m' / 64) gx <= 4 kNumCU partials of
// 64 x 16 ceil(b' / 16), update ceil(b' / 16) gx <= per_cu(m') kNumCU partials of m' x 16.
extern "C" long clo_basis_ws_bytes(long D, int m, int b) {
  if (D < 0 || m < 1 || m > BS_MAX_M || b < 1 || b > BS_MAX_B) return 0;
  long most = 4L * kNumCU * 64 * 16 * cdiv(b, 16);
  for (int mt = 1; mt <= 16; mt *= 2) {
    const long mm = std::min(m, 64 * mt);
    most = std::max(most, (long)update_per_cu(mt) * kNumCU * mm * 16);
  }
  return most * (long)sizeof(double);
}

extern "C" int clo_basis_project_f64(double *C, long ldc, const float *Q, long ldq, int m, const float *W, long ldw,
                                     int b, long D, void *ws, void *stream) {
  CLO_REQUIRE(m >= 1 && m <= BS_MAX_M && b >= 1 && b <= BS_MAX_B && D >= 0,
              "clo_basis_project_f64: needs 1 <= m <= 1024, 1 <= b <= 64, D >= 0");
  CLO_REQUIRE(C && ws && ldc >= b && ldq >= m && ldw >= b, "clo_basis_project_f64: bad operand");
  CLO_REQUIRE(D == 0 || (Q && W), "clo_basis_project_f64: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ProjArgs a{};
  a.Q = Q; a.W = W; a.ldq = ldq; a.ldw = ldw; a.D = D; a.m = m; a.b = b;
  a.vecq = (m % 4 == 0 && ldq % 4 == 0 && aligned16(Q)) ? 1 : 0;
  a.vecw = (b % 4 == 0 && ldw % 4 == 0 && aligned16(W)) ? 1 : 0;
  a.gx = project_gx(D, m);
  a.slab = static_cast<double *>(ws);
  const int NJ = (int)cdiv(b, 16);
  const dim3 grid(a.gx, (unsigned)cdiv(m, 64));
  switch (NJ) {
    case 1: hipLaunchKernelGGL(basis_project_kernel<1>, grid, dim3(BS_THREADS), 0, st, a); break;
    case 2: hipLaunchKernelGGL(basis_project_kernel<2>, grid, dim3(BS_THREADS), 0, st, a); break;
    case 3: hipLaunchKernelGGL(basis_project_kernel<3>, grid, dim3(BS_THREADS), 0, st, a); break;
    default: hipLaunchKernelGGL(basis_project_kernel<4>, grid, dim3(BS_THREADS), 0, st, a); break;
  }
  CLO_CHECK_LAUNCH("basis_project_kernel");
  hipLaunchKernelGGL(basis_reduce_kernel, dim3(m, 1), dim3(BS_THREADS), 0, st, C, ldc, a.slab, a.gx, 64, 16 * NJ, b, 1);
  CLO_CHECK_LAUNCH("basis_reduce_kernel");
  return CLO_OK;
}

extern "C" int clo_basis_update_f32(float *W, long ldw, const float *Q, long ldq, int m, const double *C, long ldc,
                                    int b, double *C2, long ldc2, long D, void *ws, void *stream) {
  CLO_REQUIRE(m >= 1 && m <= BS_MAX_M && b >= 1 && b <= BS_MAX_B && D >= 0,
              "clo_basis_update_f32: needs 1 <= m <= 1024, 1 <= b <= 64, D >= 0");
  CLO_REQUIRE(C && ldc >= b && ldq >= m && ldw >= b, "clo_basis_update_f32: bad operand");
  CLO_REQUIRE(!C2 || (ws && ldc2 >= b), "clo_basis_update_f32: C2 needs ws and ldc2 >= b");
  CLO_REQUIRE(D == 0 || (Q && W), "clo_basis_update_f32: null pointer");
  hipStream_t st = (hipStream_t)stream;
  UpdArgs a{};
  a.out = W; a.W = W; a.Q = Q; a.C = C; a.slab = C2 ? static_cast<double *>(ws) : nullptr;
  a.ldo = ldw; a.ldw = ldw; a.ldq = ldq; a.ldc = ldc; a.D = D; a.m = m; a.n = b; a.alpha = -1.f;
  a.vecq = (m % 4 == 0 && ldq % 4 == 0 && aligned16(Q)) ? 1 : 0;
  a.gx = update_gx(D, m, b);
  if (int rc = launch_update(a, st)) return rc;
  if (C2) {
    hipLaunchKernelGGL(basis_reduce_kernel, dim3(m, (unsigned)cdiv(b, 16)), dim3(BS_THREADS), 0, st, C2, ldc2, a.slab,
                       a.gx, m, 16, b, 0);
    CLO_CHECK_LAUNCH("basis_reduce_kernel");
  }
  return CLO_OK;
}

extern "C" int clo_basis_combine_f32(float *Y, long ldy, const float *Q, long ldq, int m, const double *S, long lds,
                                     int p, long D, void *stream) {
  CLO_REQUIRE(m >= 1 && m <= BS_MAX_M && p >= 1 && p <= BS_MAX_P && D >= 0,
              "clo_basis_combine_f32: needs 1 <= m, p <= 1024, D >= 0");
  CLO_REQUIRE(S && lds >= p && ldq >= m && ldy >= p, "clo_basis_combine_f32: bad operand");
  CLO_REQUIRE(D == 0 || (Q && Y), "clo_basis_combine_f32: null pointer");
  if (D == 0) return CLO_OK;
  UpdArgs a{};
  a.out = Y; a.W = nullptr; a.Q = Q; a.C = S; a.slab = nullptr;
  a.ldo = ldy; a.ldq = ldq; a.ldc = lds; a.D = D; a.m = m; a.n = p; a.alpha = 1.f;
  a.vecq = (m % 4 == 0 && ldq % 4 == 0 && aligned16(Q)) ? 1 : 0;
  a.gx = update_gx(D, m, p);
  return launch_update(a, (hipStream_t)stream);
}
