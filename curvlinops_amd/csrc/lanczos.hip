// Three-term Lanczos recurrence for K independent chains (spectrum.py, Papyan 2020 algorithm 2), one step in two
// streaming passes over [D, K] blocks in the package's K-trailing layout (row-major, K contiguous).
//
// The division by beta is deferred: a block is stored UNNORMALISED together with a per-column device scale s
// (v = s u), and since the operator is linear the product of the stored block is scaled the same way
// (A v = s A u).  Step m, column k, with W = A U:
//   pass 1:  w = s_cur W - beta_prev s_prev P;    alpha = <w, s_cur U>          reads W, U, P          12 B / element
//   pass 2:  w -= alpha s_cur U;   P <- w;        beta = ||w||, s_next = 1/beta  reads W, U, P, writes P 16 B / element
// so one step moves 28 D K bytes in two launches (the unfused torch restatement of the reference moves ~68 D bytes per
// chain in eight).  Both passes form the same float32 w; the reductions accumulate exact float32 products in float64,
// block partials in a fixed order, and the LAST block to finish (integer ticket, no float atomics) adds the partials in
// a fixed order: results are bit-identical on repeat.  Pass 1 can also store the normalised current vector s_cur U into a
// strided second copy (one column of a Krylov basis).
#include "clo_common.h"

namespace clo {
namespace {

constexpr int LZ_THREADS = 256;
constexpr int LZ_MAX_BLOCKS = 512;
constexpr int LZ_UNROLL = 4;
constexpr long LZ_TICKET_BYTES = 256;   // ticket word, padded so the partials start 256-byte aligned

constexpr int LZ_FIRST = 1, LZ_LAST = 2;

// blocks: every block ends with a device-scope release + ticket atomic, and a step slows down as the grid grows (C2,
// K = 1: 65 / 86 / 157 / 206 us per step at 256 / 512 / 1024 / 2048 blocks; K = 8 and 32 are fastest at 512), so the
// grid is kept small and each thread keeps LZ_UNROLL rows (K = 1: float4 groups of four rows) in flight instead
inline int lz_blocks(long D, int K) {
  const long rows = K == 1 ? 4L * LZ_THREADS : LZ_THREADS / K;
  const long cap = K == 1 ? LZ_MAX_BLOCKS / 2 : LZ_MAX_BLOCKS;
  return (int)std::max<long>(1, std::min<long>(cap, cdiv(D, rows * LZ_UNROLL)));
}

// PASS 1: alpha; PASS 2: update, next residual, beta.  Thread t owns column t % K of rows t / K, t / K + R, ...
// (R = 256 / K rows per sweep; a sweep is R K consecutive floats, so the loads of a wave are contiguous).
template <int PASS, bool FIRST>
__global__ __launch_bounds__(LZ_THREADS) void lanczos_pass_kernel(
    const float *__restrict__ W, const float *__restrict__ U, float *P, long D, int K, const double *__restrict__ s_cur,
    const double *__restrict__ s_prev, const double *__restrict__ beta_prev, double *alpha, double *__restrict__ beta,
    double *__restrict__ s_next, float *__restrict__ out, long ldo, int last, double *part, unsigned *ticket) {
  __shared__ double s_acc[LZ_THREADS];
  __shared__ bool s_last;
  const int t = threadIdx.x;
  const int R = LZ_THREADS / K;
  const bool active = t < R * K;
  const int k = active ? t % K : 0;
  const int r = t / K;

  const float a = (float)s_cur[k];
  const float b = FIRST ? 0.f : (float)(beta_prev[k] * s_prev[k]);
  const float c = PASS == 2 ? (float)(alpha[k] * s_cur[k]) : 0.f;

  double acc = 0.0;
  // K = 1 with 16-byte aligned blocks: four consecutive rows per float4 load
  const bool vec = K == 1 && (((uintptr_t)W | (uintptr_t)U | (uintptr_t)P) & 15u) == 0;
  if (vec) {
    const long n4 = D / 4, stride = (long)gridDim.x * LZ_THREADS;
    long q = (long)blockIdx.x * LZ_THREADS + t;
    for (; q < n4; q += LZ_UNROLL * stride) {
      float4 wv[LZ_UNROLL], uv[LZ_UNROLL], pv[LZ_UNROLL];
#pragma unroll
      for (int j = 0; j < LZ_UNROLL; ++j) {
        const long qj = q + j * stride;
        if (qj < n4) {
          wv[j] = reinterpret_cast<const float4 *>(W)[qj];
          uv[j] = reinterpret_cast<const float4 *>(U)[qj];
          pv[j] = FIRST ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4 *>(P)[qj];
        }
      }
#pragma unroll
      for (int j = 0; j < LZ_UNROLL; ++j) {
        const long qj = q + j * stride;
        if (qj >= n4) break;
        float w[4] = {a * wv[j].x, a * wv[j].y, a * wv[j].z, a * wv[j].w};
        const float u[4] = {uv[j].x, uv[j].y, uv[j].z, uv[j].w}, p[4] = {pv[j].x, pv[j].y, pv[j].z, pv[j].w};
        double s4 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (!FIRST) w[i] = fmaf(-b, p[i], w[i]);
          if (PASS == 1) {
            s4 += (double)w[i] * u[i];
            if (out) out[(4 * qj + i) * ldo] = a * u[i];
          } else {
            w[i] = fmaf(-c, u[i], w[i]);
            s4 += (double)w[i] * w[i];
          }
        }
        if (PASS == 2 && !last) reinterpret_cast<float4 *>(P)[qj] = make_float4(w[0], w[1], w[2], w[3]);
        acc += s4;
      }
    }
    for (long row = 4 * n4 + (long)blockIdx.x * LZ_THREADS + t; row < D; row += stride) {
      const float u = U[row];
      float w = FIRST ? a * W[row] : fmaf(-b, P[row], a * W[row]);
      if (PASS == 1) {
        acc += (double)w * u;
        if (out) out[row * ldo] = a * u;
      } else {
        w = fmaf(-c, u, w);
        if (!last) P[row] = w;
        acc += (double)w * w;
      }
    }
  } else if (active) {
    const long rstride = (long)gridDim.x * R;
    long row = (long)blockIdx.x * R + r;
    // LZ_UNROLL rows in flight per thread: all loads first, then the arithmetic
    for (; row + (LZ_UNROLL - 1) * rstride < D; row += LZ_UNROLL * rstride) {
      float wv[LZ_UNROLL], uv[LZ_UNROLL], pv[LZ_UNROLL];
#pragma unroll
      for (int q = 0; q < LZ_UNROLL; ++q) {
        const long e = (row + q * rstride) * K + k;
        wv[q] = W[e];
        uv[q] = U[e];
        pv[q] = FIRST ? 0.f : P[e];
      }
#pragma unroll
      for (int q = 0; q < LZ_UNROLL; ++q) {
        float w = FIRST ? a * wv[q] : fmaf(-b, pv[q], a * wv[q]);
        if (PASS == 1) {
          acc += (double)w * uv[q];
          if (out) out[(row + q * rstride) * ldo + k] = a * uv[q];
        } else {
          w = fmaf(-c, uv[q], w);
          if (!last) P[(row + q * rstride) * K + k] = w;
          acc += (double)w * w;
        }
      }
    }
    for (; row < D; row += rstride) {
      const long e = row * K + k;
      const float u = U[e];
      float w = FIRST ? a * W[e] : fmaf(-b, P[e], a * W[e]);
      if (PASS == 1) {
        acc += (double)w * u;
        if (out) out[row * ldo + k] = a * u;
      } else {
        w = fmaf(-c, u, w);
        if (!last) P[e] = w;
        acc += (double)w * w;
      }
    }
  }

  // block partial of every column, rows added in a fixed order
  s_acc[t] = acc;
  __syncthreads();
  if (t < K) {
    double sum = 0.0;
    for (int q = 0; q < R; ++q) sum += s_acc[q * K + t];
    part[(long)blockIdx.x * K + t] = sum;
    __threadfence();
  }
  __syncthreads();
  if (t == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;

  // last block: partials of all blocks, R interleaved groups per column, then the groups in order
  __threadfence();
  const int nb = gridDim.x;
  double sum = 0.0;
  if (active)
    for (int blk = r; blk < nb; blk += R)
      sum += __hip_atomic_load(&part[(long)blk * K + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  s_acc[t] = sum;
  __syncthreads();
  if (t < K) {
    double tot = 0.0;
    for (int q = 0; q < R; ++q) tot += s_acc[q * K + t];
    if (PASS == 1) {
      alpha[t] = s_cur[t] * tot;
    } else {
      const double bt = sqrt(tot);
      beta[t] = bt;
      s_next[t] = 1.0 / bt;   // (beta = 0 is not special-cased, as in the reference: the next block is inf / nan)
    }
  }
  if (t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next pass
}

template <int PASS>
int launch_pass(bool first, int nb, hipStream_t st, const float *W, const float *U, float *P, long D, int K,
                const double *s_cur, const double *s_prev, const double *beta_prev, double *alpha, double *beta,
                double *s_next, float *out, long ldo, int last, double *part, unsigned *ticket) {
  if (first)
    hipLaunchKernelGGL((lanczos_pass_kernel<PASS, true>), dim3(nb), dim3(LZ_THREADS), 0, st, W, U, P, D, K, s_cur, s_prev,
                       beta_prev, alpha, beta, s_next, out, ldo, last, part, ticket);
  else
    hipLaunchKernelGGL((lanczos_pass_kernel<PASS, false>), dim3(nb), dim3(LZ_THREADS), 0, st, W, U, P, D, K, s_cur,
                       s_prev, beta_prev, alpha, beta, s_next, out, ldo, last, part, ticket);
  CLO_CHECK_LAUNCH("lanczos_pass_kernel");
  return CLO_OK;
}

}  // namespace
}  // namespace clo

using namespace clo;

extern "C" long clo_lanczos_ws_bytes(long D, int K) {
  if (D < 0 || K < 1 || K > 64) return -1;
  return LZ_TICKET_BYTES + (long)lz_blocks(D, K) * K * (long)sizeof(double);
}

extern "C" int clo_lanczos_step_f32(const float *W, const float *U, float *P, long D, int K, const double *s_cur,
                                    const double *s_prev, const double *beta_prev, double *alpha, double *beta,
                                    double *s_next, float *out, long ldo, int flags, void *ws, void *stream) {
  CLO_REQUIRE(D >= 0, "clo_lanczos_step_f32: negative D");
  CLO_REQUIRE(K >= 1 && K <= 64, "clo_lanczos_step_f32: K = %d outside [1, 64]", K);
  CLO_REQUIRE((flags & ~(LZ_FIRST | LZ_LAST)) == 0, "clo_lanczos_step_f32: unknown flags %d", flags);
  const bool first = flags & LZ_FIRST, last = flags & LZ_LAST;
  CLO_REQUIRE(s_cur && alpha && beta && s_next && ws, "clo_lanczos_step_f32: null pointer");
  CLO_REQUIRE(first || (s_prev && beta_prev), "clo_lanczos_step_f32: s_prev / beta_prev required after step 0");
  CLO_REQUIRE(D == 0 || (W && U && ((first && last) || P)), "clo_lanczos_step_f32: null block pointer");
  CLO_REQUIRE(!out || ldo >= K, "clo_lanczos_step_f32: ldo = %ld < K = %d", ldo, K);
  CLO_REQUIRE(((uintptr_t)ws & 7u) == 0, "clo_lanczos_step_f32: ws not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = lz_blocks(D, K);
  unsigned *ticket = (unsigned *)ws;
  double *part = (double *)((char *)ws + LZ_TICKET_BYTES);
  int rc = launch_pass<1>(first, nb, st, W, U, P, D, K, s_cur, s_prev, beta_prev, alpha, beta, s_next, out, ldo, last,
                          part, ticket);
  if (rc != CLO_OK) return rc;
  return launch_pass<2>(first, nb, st, W, U, P, D, K, s_cur, s_prev, beta_prev, alpha, beta, s_next, nullptr, 0, last,
                        part, ticket);
}
