// kg_supervisor.hip — Learner/DeepSupervisor (supervised learning of
// feed-forward networks, float32) on MI355X.
//
// One training step is a chain of launches on the handle's stream with no
// host round trip: the forward pass (one product per Linear layer, the
// following elementwise activation in its epilogue), the loss gradient, the
// Output layer's backward, per Linear layer the weight gradient (split over
// the batch where the output is small), the bias gradient and the data
// gradient (the preceding activation's derivative in its epilogue), the L2
// term and the optimizer.  `steps` steps are enqueued back to back and the
// loss is read once, after the last.
//
// The three products share one kernel, k_sv_gemm: C[m][n] = sum_k A(m,k) B(n,k)
// on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation), a
// 128 x 128 tile per workgroup of four waves (64 x 64 per wave: 2 x 2 MFMA
// tiles, four independent accumulators), k in steps of 16 through two LDS
// buffers with the next step's global loads in flight during the current
// step's MFMAs.  Either operand may be contiguous along k or along its own
// index; full, 16-byte aligned tiles load as float4, everything else (edges,
// odd strides, the weights' unaligned offset in the hyperparameter vector)
// element by element with zero fill.
//
// Every reduction has a fixed order: the split-batch partials of a weight
// gradient and the bias gradient's are summed slab after slab, the loss by a
// fixed tree.  There are no floating-point atomics.
//
// Reference (paths relative to the korali root):
//   DeepSupervisor::initialize / runGeneration / getEvaluation
//                                   solver/learner/deepSupervisor/deepSupervisor.cpp.base
//   Linear                          neuralNetwork/layer/linear/linear.cpp.base:219-232, :284-292, :337-350
//   Activation ("Korali" engine)    neuralNetwork/layer/activation/activation.cpp.base:147-209, :270-314
//   Output                          neuralNetwork/layer/output/output.cpp.base:115-232
//   logSumExp                       auxiliar/math.hpp:205-225
//   optimizers                      solver/learner/deepSupervisor/optimizers/f{Adam,AdaBelief,MadGrad,RMSProp,Adagrad}.cpp
// The NumPy restatement is tests/supervisor_ref.py (test infrastructure only).
#include "kg_common.hpp"
#include "../../include/korali_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace kg {
namespace sv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BK = 16, LDP = BM + 4;  // tile edge, k-step, LDS row stride (floats; 16-byte rows)
constexpr int FN_NONE = -1;
enum : int { SV_FORWARD = 0, SV_DGRAD = 1, SV_STORE = 2 };

// activation.cpp.base:147-209, one element
__device__ __forceinline__ float act_fwd(int fn, float x, float alpha, float beta) {
  switch (fn) {
    case KG_SV_TANH: return tanhf(x);
    case KG_SV_RELU: return x > 0.0f ? x : x * alpha;
    case KG_SV_LOGISTIC: return 1.0f / (1.0f + expf(-x));
    case KG_SV_SOFTRELU: return logf(1.0f + expf(x));
    case KG_SV_SOFTSIGN: return x / (1.0f + fabsf(x));
    case KG_SV_ELINEAR: return x * alpha + beta;
    case KG_SV_LOG: return logf(x);
    default: return x;
  }
}

// activation.cpp.base:270-314, one element: g the gradient with respect to
// the activation's value y, z the activation's input
__device__ __forceinline__ float act_bwd(int fn, float g, float y, float z, float alpha) {
  switch (fn) {
    case KG_SV_TANH: return g * (1.0f - y * y);
    case KG_SV_RELU: return z > 0.0f ? g : g * alpha;
    case KG_SV_LOGISTIC:
    case KG_SV_SOFTMAX: return g * y * (1.0f - y);
    case KG_SV_SOFTRELU: {
      const float e = expf(y);
      return g * (e - 1.0f) / e;
    }
    case KG_SV_SOFTSIGN: return g / ((1.0f + fabsf(y)) * (1.0f + fabsf(y)));
    case KG_SV_ELINEAR: return g * alpha;
    case KG_SV_LOG: return g / z;
    default: return g;
  }
}

struct Gemm {
  int M, N, K, chunk;  // chunk: k per blockIdx.z (a multiple of BK)
  const float *A;
  long long sam, sak;
  const float *B;
  long long sbn, sbk;
  float *C;  // SV_STORE: slab blockIdx.z at C + z M N
  long long ldc;
  int vecA, vecB;     // the operand's stride and base allow float4 loads
  const float *bias;  // SV_FORWARD
  float *C2;          // SV_FORWARD: the activation's values (fn != FN_NONE)
  const float *Y, *Z; // SV_DGRAD: the preceding activation's values and its input
  int fn;
  float alpha, beta;
};

// One operand's 128 x 16 panel: global -> registers.  KC: contiguous along k.
template <bool KC>
__device__ __forceinline__ void load_panel(float (&r)[8], const float *__restrict__ P, long long sr, long long sk, int r0,
                                           int R, int k0, int kend, bool fast, int t) {
  if (fast) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int e = t + 256 * q;
      float4 v;
      if (KC) v = *reinterpret_cast<const float4 *>(P + (long long)(r0 + (e >> 2)) * sr + k0 + 4 * (e & 3));
      else v = *reinterpret_cast<const float4 *>(P + (long long)(k0 + (e >> 5)) * sk + r0 + 4 * (e & 31));
      r[4 * q] = v.x, r[4 * q + 1] = v.y, r[4 * q + 2] = v.z, r[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int e = t + 256 * q;
      const int k = KC ? (e & 15) : (e >> 7), row = KC ? (e >> 4) : (e & 127);
      const int gr = r0 + row, gk = k0 + k;
      r[q] = (gr < R && gk < kend) ? P[(long long)gr * sr + (long long)gk * sk] : 0.0f;
    }
  }
}

template <bool KC>
__device__ __forceinline__ void store_panel(float (*S)[LDP], const float (&r)[8], bool fast, int t) {
  if (fast) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int e = t + 256 * q;
      if (KC) {
        const int row = e >> 2, k = 4 * (e & 3);
        S[k][row] = r[4 * q], S[k + 1][row] = r[4 * q + 1], S[k + 2][row] = r[4 * q + 2], S[k + 3][row] = r[4 * q + 3];
      } else {
        *reinterpret_cast<float4 *>(&S[e >> 5][4 * (e & 31)]) = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int e = t + 256 * q;
      const int k = KC ? (e & 15) : (e >> 7), row = KC ? (e >> 4) : (e & 127);
      S[k][row] = r[q];
    }
  }
}

template <int EP, bool AKC, bool BKC>
__global__ __launch_bounds__(256) void k_sv_gemm(Gemm g) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDP];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BM;
  const int kbeg = blockIdx.z * g.chunk, kend = min(g.K, kbeg + g.chunk);
  const bool fullA = g.vecA && m0 + BM <= g.M, fullB = g.vecB && n0 + BM <= g.N;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
  float ra[8], rb[8];
  bool fa = fullA && kbeg + BK <= kend, fb = fullB && kbeg + BK <= kend;
  load_panel<AKC>(ra, g.A, g.sam, g.sak, m0, g.M, kbeg, kend, fa, t);
  load_panel<BKC>(rb, g.B, g.sbn, g.sbk, n0, g.N, kbeg, kend, fb, t);
  store_panel<AKC>(As[0], ra, fa, t);
  store_panel<BKC>(Bs[0], rb, fb, t);
  __syncthreads();
  int cur = 0;
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) {
      fa = fullA && k0 + 2 * BK <= kend, fb = fullB && k0 + 2 * BK <= kend;
      load_panel<AKC>(ra, g.A, g.sam, g.sak, m0, g.M, k0 + BK, kend, fa, t);
      load_panel<BKC>(rb, g.B, g.sbn, g.sbk, n0, g.N, k0 + BK, kend, fb, t);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
      const float a0 = As[cur][kk + lh][wm * 64 + li], a1 = As[cur][kk + lh][wm * 64 + 32 + li];
      const float b0 = Bs[cur][kk + lh][wn * 64 + li], b1 = Bs[cur][kk + lh][wn * 64 + 32 + li];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (more) {
      store_panel<AKC>(As[cur ^ 1], ra, fa, t);
      store_panel<BKC>(Bs[cur ^ 1], rb, fb, t);
    }
    __syncthreads();
    cur ^= 1;
  }
  // C/D of the 32x32 forms: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float *C = g.C;
  if (EP == SV_STORE) C += (long long)blockIdx.z * g.M * g.N;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int col = n0 + wn * 64 + j * 32 + li;
      if (col >= g.N) continue;
      float bias = 0.0f;
      if (EP == SV_FORWARD) bias = g.bias[col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row >= g.M) continue;
        const long long o = (long long)row * g.ldc + col;
        float v = acc[i][j][r];
        if (EP == SV_FORWARD) {
          v = v + bias;
          C[o] = v;
          if (g.fn != FN_NONE) g.C2[o] = act_fwd(g.fn, v, g.alpha, g.beta);
        } else if (EP == SV_DGRAD) {
          if (g.fn != FN_NONE) v = act_bwd(g.fn, v, g.Y[o], g.Z[o], g.alpha);
          C[o] = v;
        } else {
          C[o] = v;
        }
      }
    }
}

// dst[i] = part[0][i] + part[1][i] + ..., slab after slab
__global__ void k_sv_reduce(long long n, int slabs, const float *__restrict__ part, float *__restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int q = 1; q < slabs; q++) s += part[(long long)q * n + i];
  dst[i] = s;
}

// part[blockIdx.y][o] = sum of G[b][o] over the slab's rows, in row order
// (linear.cpp.base:347-349 sums all rows in this order)
__global__ void k_sv_bias_part(int Bn, int OC, int rows, const float *__restrict__ G, float *__restrict__ part) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= OC) return;
  const int b0 = blockIdx.y * rows, b1 = min(Bn, b0 + rows);
  float s = 0.0f;
  for (int b = b0; b < b1; b++) s += G[(long long)b * OC + o];
  part[(long long)blockIdx.y * OC + o] = s;
}

__global__ void k_sv_act_fwd(long long n, int fn, float alpha, float beta, const float *__restrict__ z,
                             float *__restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = act_fwd(fn, z[i], alpha, beta);
}

__global__ void k_sv_act_bwd(long long n, int fn, float alpha, const float *__restrict__ g, const float *__restrict__ y,
                             const float *__restrict__ z, float *__restrict__ gz) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) gz[i] = act_bwd(fn, g[i], y[i], z[i], alpha);
}

// Softmax (activation.cpp.base:200-207, logSumExp math.hpp:205-225), a wave
// per row: the maximum, the sum of exp(x - max) (lane sums, then a fixed
// butterfly), exp(x - (max + log sum)).
__global__ void k_sv_softmax(int rows, int OC, const float *__restrict__ z, float *__restrict__ y) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *x = z + (long long)row * OC;
  float mx = -INFINITY;
  for (int j = lane; j < OC; j += 64) mx = fmaxf(mx, x[j]);
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float lse;
  if (isinf(mx)) {
    lse = mx;
  } else {
    float s = 0.0f;
    for (int j = lane; j < OC; j += 64) s += expf(x[j] - mx);
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    lse = mx + logf(s);
  }
  for (int j = lane; j < OC; j += 64) y[(long long)row * OC + j] = expf(x[j] - lse);
}

// Output layer, forward (output.cpp.base:141-162; the double stages are the
// reference's own: `1. / (1. + ...)`, `0.5 * (x + std::sqrt(1. + x * x))`)
__global__ void k_sv_out_fwd(long long n, int OC, const float *__restrict__ src, float *__restrict__ out,
                             const float *__restrict__ scale, const float *__restrict__ shift,
                             const int *__restrict__ mask) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i % OC);
  float x = src[i];
  const int m = mask ? mask[j] : KG_SV_IDENTITY;
  if (m == KG_SV_ABSOLUTE) x = fabsf(x);
  if (m == KG_SV_SIGMOID) x = (float)(1.0 / (1.0 + (double)expf(-x)));
  if (m == KG_SV_SOFTPLUS) x = (float)(0.5 * ((double)x + sqrt(1.0 + (double)(x * x))));
  if (m == KG_SV_MASK_TANH) x = tanhf(x);
  if (scale) x *= scale[j];
  if (shift) x += shift[j];
  out[i] = x;
}

// Output layer, backward (output.cpp.base:175-212)
__global__ void k_sv_out_bwd(long long n, int OC, const float *__restrict__ out, const float *__restrict__ src,
                             const float *__restrict__ G, float *__restrict__ dst, const float *__restrict__ scale,
                             const float *__restrict__ shift, const int *__restrict__ mask) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i % OC);
  float x = out[i], g = G[i];
  if (shift) x = x - shift[j];
  if (scale) {
    x = x / scale[j];
    g = g * scale[j];
  }
  const int m = mask ? mask[j] : KG_SV_IDENTITY;
  if (m == KG_SV_ABSOLUTE)
    if (signbit(x) != signbit(src[i])) g = -g;
  if (m == KG_SV_MASK_TANH) g = g * (1.0f - x * x);
  if (m == KG_SV_SOFTPLUS) {
    const float nnx = (float)((double)x - 0.25 / (double)x);
    g = (float)((double)g * 0.5 * (1.0 + (double)(nnx / sqrtf(nnx * nnx + 1.0f))));
  }
  if (m == KG_SV_SIGMOID) g = (float)((double)(g * x) * (1.0 - (double)x));
  dst[i] = g;
}

// g = solution - output (deepSupervisor.cpp.base:124-126) and, where `part`
// is given, the block's sum of g^2 by a fixed tree (:132-135)
constexpr int LOSS_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_sv_mse(long long n, const float *__restrict__ sol, const float *__restrict__ out,
                                                float *__restrict__ g, float *__restrict__ part) {
  __shared__ float red[256];
  float s = 0.0f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = sol[i] - out[i];
    g[i] = d;
    s += d * d;
  }
  if (!part) return;
  red[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// loss = (sum of the blocks' sums, same tree) / (N * 2) (:136)
__global__ __launch_bounds__(256) void k_sv_loss(int blocks, const float *__restrict__ part, float rows,
                                                 float *__restrict__ loss) {
  __shared__ float red[256];
  red[threadIdx.x] = (int)threadIdx.x < blocks ? part[threadIdx.x] : 0.0f;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0] / (rows * 2.0f);
}

// deepSupervisor.cpp.base:151-152
__global__ void k_sv_l2(long long n, float importance, const float *__restrict__ theta, float *__restrict__ grad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) grad[i] -= importance * theta[i];
}

// fAdam.cpp:78-90
__global__ void k_sv_adam(long long n, float eta, float f1, float f2, float *__restrict__ theta,
                          const float *__restrict__ grad, float *__restrict__ m1, float *__restrict__ m2) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-08f, nb1 = 1.0f - beta1, nb2 = 1.0f - beta2, gr = grad[i];
  const float a = beta1 * m1[i] - nb1 * gr;
  const float b = beta2 * m2[i] + nb2 * gr * gr;
  m1[i] = a, m2[i] = b;
  theta[i] -= eta / (sqrtf(b * f2) + eps) * a * f1;
}

// fAdaBelief.cpp:35-52
__global__ void k_sv_adabelief(long long n, float eta, float f1, float f2, float *__restrict__ theta,
                               const float *__restrict__ grad, float *__restrict__ m1, float *__restrict__ sc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-08f, nb1 = 1.0f - beta1, nb2 = 1.0f - beta2, gr = grad[i];
  const float a = beta1 * m1[i] - nb1 * gr;
  m1[i] = a;
  const float corrected = a * f1, diff = gr + a;
  const float c = beta2 * sc[i] + nb2 * diff * diff;
  sc[i] = c;
  theta[i] -= eta / (sqrtf(c * f2) + eps) * corrected;
}

// fMadGrad.cpp:62-71 (the optimizer's _initialValues are zeros)
__global__ void k_sv_madgrad(long long n, float eta, float *__restrict__ theta, const float *__restrict__ grad,
                             float *__restrict__ s, float *__restrict__ v, float *__restrict__ z) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float eps = 1e-08f, momentum = 0.9f, gr = grad[i];
  const float si = s[i] + eta * gr, vi = v[i] - eta * (gr * gr);
  const float zi = 0.0f - (1.0f / (cbrtf(vi) + eps)) * si;
  s[i] = si, v[i] = vi, z[i] = zi;
  theta[i] = (1.0f - momentum) * theta[i] + momentum * zi;
}

// fRMSProp.cpp:63-65
__global__ void k_sv_rmsprop(long long n, float eta, float *__restrict__ theta, const float *__restrict__ grad,
                             float *__restrict__ r, float *__restrict__ v) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float eps = 1e-08f, decay = 0.999f, gr = grad[i];
  const float ri = (1.0f - decay) * (gr * gr) + decay * r[i];
  const float vi = (eta / (sqrtf(ri) + eps)) * -gr;
  r[i] = ri, v[i] = vi;
  theta[i] = theta[i] - vi;
}

// fAdagrad.cpp:49-50
__global__ void k_sv_adagrad(long long n, float eta, float *__restrict__ theta, const float *__restrict__ grad,
                             float *__restrict__ s) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float eps = 1e-08f, gr = grad[i];
  const float si = s[i] + (gr * gr);
  s[i] = si;
  theta[i] += (eta / sqrtf(si + eps)) * gr;
}

struct Layer {
  int type = KG_SV_LINEAR, fn = FN_NONE;
  float alpha = 0.0f, beta = 0.0f;
  size_t oc = 0, ic = 0, woff = 0;  // Linear: the offset of [W, b] in the hyperparameters
  int splits = 1, chunk = 0;        // Linear: the weight gradient's split over the batch
};

}  // namespace sv
}  // namespace kg

using namespace kg;
using namespace kg::sv;

struct kg_supervisor_s {
  int device = 0;
  hipStream_t stream = nullptr;
  size_t IC = 0, OC = 0, NB[2] = {0, 0};
  int pipes = 1;  // 1: both batch sizes are equal and share the buffers
  // [0] the input, [1 .. n] the given layers, [n + 1] the Output layer
  std::vector<Layer> L;
  size_t nh = 0;
  float *theta = nullptr, *grad = nullptr, *state[3] = {nullptr, nullptr, nullptr};
  std::vector<std::string> stateNames;
  float *trainX = nullptr, *sol = nullptr, *G0 = nullptr;
  std::vector<float *> out[2];  // per pipeline and layer (out[p][0]: an evaluation's input)
  const float *in[2] = {nullptr, nullptr};  // the input of the pipeline's last forward pass
  std::vector<float *> G;       // training pipeline: the gradient with respect to a layer's values
  float *ws = nullptr, *bpart = nullptr, *lpart = nullptr, *lossDev = nullptr, *lossHost = nullptr;
  float *scale = nullptr, *shift = nullptr;
  int *mask = nullptr;
  int optimizer = 0, loss = 0, l2 = 0;
  float eta = 0.0f, l2imp = 0.0f, b1p = 1.0f, b2p = 1.0f, currentLoss = 0.0f;
  size_t evals = 0;
  bool forwarded = false, haveData = false;
  int biasSlabs = 1, biasRows = 1;
  int prof = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::map<std::string, std::pair<double, size_t>> totals;
};

namespace {

// a stage's launches between two events; a profiled stage is waited for
struct SvStage {
  kg_supervisor_s *h;
  const char *name;
  SvStage(kg_supervisor_s *h_, const char *n) : h(h_), name(n) {
    if (h->prof) (void)hipEventRecord(h->e0, h->stream);
  }
  ~SvStage() {
    if (!h->prof) return;
    float ms = 0.0f;
    if (hipEventRecord(h->e1, h->stream) == hipSuccess && hipEventSynchronize(h->e1) == hipSuccess &&
        hipEventElapsedTime(&ms, h->e0, h->e1) == hipSuccess) {
      auto &t = h->totals[name];
      t.first += ms, t.second += 1;
    }
  }
};

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned sv_blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// C[M x N] = sum_k A(m,k) B(n,k); splits > 1: slabs at C
template <int EP>
int sv_gemm(kg_supervisor_s *h, Gemm g, int splits) {
  const bool akc = g.sak == 1, bkc = g.sbk == 1;
  // float4 loads: along k for a k-contiguous operand (row stride), along the row index otherwise (k stride)
  g.vecA = aligned16(g.A) && (akc ? g.sam % 4 == 0 : (g.sam == 1 && g.sak % 4 == 0));
  g.vecB = aligned16(g.B) && (bkc ? g.sbn % 4 == 0 : (g.sbn == 1 && g.sbk % 4 == 0));
  dim3 grid((g.N + BM - 1) / BM, (g.M + BM - 1) / BM, splits), block(256);
  if (akc && bkc) hipLaunchKernelGGL((k_sv_gemm<EP, true, true>), grid, block, 0, h->stream, g);
  else if (akc && !bkc) hipLaunchKernelGGL((k_sv_gemm<EP, true, false>), grid, block, 0, h->stream, g);
  else if (!akc && !bkc) hipLaunchKernelGGL((k_sv_gemm<EP, false, false>), grid, block, 0, h->stream, g);
  else hipLaunchKernelGGL((k_sv_gemm<EP, false, true>), grid, block, 0, h->stream, g);
  KG_HIP(hipGetLastError());
  return 0;
}

// the forward pass of pipeline p over `rows` rows from X (device)
int sv_forward(kg_supervisor_s *h, int p, const float *X) {
  SvStage st(h, "forward");
  const int rows = (int)h->NB[p], last = (int)h->L.size() - 1;
  auto &o = h->out[p];
  h->in[p] = X;
  auto val = [&](int l) -> const float * { return l == 0 ? X : o[l]; };
  for (int l = 1; l < last; l++) {
    const Layer &ly = h->L[l];
    const long long n = (long long)rows * ly.oc;
    if (ly.type == KG_SV_LINEAR) {
      Gemm g{};
      g.M = rows, g.N = (int)ly.oc, g.K = (int)ly.ic, g.chunk = (int)((ly.ic + BK - 1) / BK * BK);
      g.A = val(l - 1), g.sam = (long long)ly.ic, g.sak = 1;
      g.B = h->theta + ly.woff, g.sbn = (long long)ly.ic, g.sbk = 1;
      g.C = o[l], g.ldc = (long long)ly.oc, g.bias = h->theta + ly.woff + ly.ic * ly.oc, g.fn = FN_NONE;
      const Layer &nx = h->L[l + 1];
      const bool fuse = l + 1 < last && nx.type == KG_SV_ACTIVATION && nx.fn != KG_SV_SOFTMAX;
      if (fuse) g.fn = nx.fn, g.alpha = nx.alpha, g.beta = nx.beta, g.C2 = o[l + 1];
      if (sv_gemm<SV_FORWARD>(h, g, 1)) return 1;
      if (fuse) l++;
    } else if (ly.fn == KG_SV_SOFTMAX) {
      hipLaunchKernelGGL(k_sv_softmax, dim3(sv_blocks(rows, 4)), dim3(256), 0, h->stream, rows, (int)ly.oc, val(l - 1), o[l]);
    } else {
      hipLaunchKernelGGL(k_sv_act_fwd, dim3(sv_blocks(n)), dim3(256), 0, h->stream, n, ly.fn, ly.alpha, ly.beta, val(l - 1), o[l]);
    }
  }
  const long long n = (long long)rows * h->OC;
  hipLaunchKernelGGL(k_sv_out_fwd, dim3(sv_blocks(n)), dim3(256), 0, h->stream, n, (int)h->OC, val(last - 1), o[last],
                     h->scale, h->shift, h->mask);
  KG_HIP(hipGetLastError());
  if (p == 0) h->forwarded = true;
  return 0;
}

// the backward pass of the training pipeline from Gout (the gradient with
// respect to the network's output, device): fills h->grad
int sv_backward(kg_supervisor_s *h, const float *Gout) {
  const int rows = (int)h->NB[0], last = (int)h->L.size() - 1;
  auto &o = h->out[0];
  auto val = [&](int l) -> const float * { return l == 0 ? h->in[0] : o[l]; };
  {
    SvStage st(h, "other");
    const long long n = (long long)rows * h->OC;
    hipLaunchKernelGGL(k_sv_out_bwd, dim3(sv_blocks(n)), dim3(256), 0, h->stream, n, (int)h->OC, o[last], val(last - 1),
                       Gout, h->G[last - 1], h->scale, h->shift, h->mask);
  }
  for (int l = last - 1; l >= 1; l--) {
    const Layer &ly = h->L[l];
    if (ly.type == KG_SV_ACTIVATION) {
      if (l - 1 == 0) continue;  // the gradient with respect to the input is not needed
      SvStage st(h, "other");
      const long long n = (long long)rows * ly.oc;
      hipLaunchKernelGGL(k_sv_act_bwd, dim3(sv_blocks(n)), dim3(256), 0, h->stream, n, ly.fn, ly.alpha, h->G[l], o[l],
                         val(l - 1), h->G[l - 1]);
      continue;
    }
    float *dW = h->grad + ly.woff, *db = dW + ly.ic * ly.oc;
    {
      // dW[o][i] = sum_b G[b][o] X[b][i] (linear.cpp.base:340-344), db (:347-349)
      SvStage st(h, "weight_gradient");
      Gemm g{};
      g.M = (int)ly.oc, g.N = (int)ly.ic, g.K = rows, g.chunk = ly.chunk;
      g.A = h->G[l], g.sam = 1, g.sak = (long long)ly.oc;
      g.B = val(l - 1), g.sbn = 1, g.sbk = (long long)ly.ic;
      g.C = ly.splits > 1 ? h->ws : dW, g.ldc = (long long)ly.ic, g.fn = FN_NONE;
      if (sv_gemm<SV_STORE>(h, g, ly.splits)) return 1;
      const long long nw = (long long)ly.oc * ly.ic;
      if (ly.splits > 1)
        hipLaunchKernelGGL(k_sv_reduce, dim3(sv_blocks(nw)), dim3(256), 0, h->stream, nw, ly.splits, h->ws, dW);
      hipLaunchKernelGGL(k_sv_bias_part, dim3(sv_blocks((long long)ly.oc), h->biasSlabs), dim3(256), 0, h->stream, rows,
                         (int)ly.oc, h->biasRows, h->G[l], h->bpart);
      hipLaunchKernelGGL(k_sv_reduce, dim3(sv_blocks((long long)ly.oc)), dim3(256), 0, h->stream, (long long)ly.oc,
                         h->biasSlabs, h->bpart, db);
    }
    if (l - 1 == 0) continue;
    const Layer &pv = h->L[l - 1];
    const bool fuse = pv.type == KG_SV_ACTIVATION && pv.fn != KG_SV_SOFTMAX && l - 2 >= 1;
    if (pv.type == KG_SV_ACTIVATION && l - 2 == 0 && pv.fn != KG_SV_SOFTMAX) {
      // an activation on the input itself: nothing below it takes a gradient
      continue;
    }
    {
      // dX = G W (linear.cpp.base:287-291), times the preceding activation's derivative
      SvStage st(h, "data_gradient");
      Gemm g{};
      g.M = rows, g.N = (int)ly.ic, g.K = (int)ly.oc, g.chunk = (int)((ly.oc + BK - 1) / BK * BK);
      g.A = h->G[l], g.sam = (long long)ly.oc, g.sak = 1;
      g.B = h->theta + ly.woff, g.sbn = 1, g.sbk = (long long)ly.ic;
      g.ldc = (long long)ly.ic, g.fn = FN_NONE;
      if (fuse) {
        g.C = h->G[l - 2], g.fn = pv.fn, g.alpha = pv.alpha, g.Y = o[l - 1], g.Z = val(l - 2);
      } else {
        g.C = h->G[l - 1];
      }
      if (sv_gemm<SV_DGRAD>(h, g, 1)) return 1;
    }
    if (fuse) l--;
  }
  KG_HIP(hipGetLastError());
  return 0;
}

int sv_optimize(kg_supervisor_s *h) {
  SvStage st(h, "optimizer");
  const long long n = (long long)h->nh;
  const dim3 grid(sv_blocks(n)), block(256);
  if (h->l2 && h->l2imp != 0.0f) hipLaunchKernelGGL(k_sv_l2, grid, block, 0, h->stream, n, h->l2imp, h->theta, h->grad);
  switch (h->optimizer) {
    case KG_SV_ADAM: {
      h->evals++;
      h->b1p *= 0.9f, h->b2p *= 0.999f;  // fAdam.cpp:69-70
      const float f1 = 1.0f / (1.0f - h->b1p), f2 = 1.0f / (1.0f - h->b2p);
      hipLaunchKernelGGL(k_sv_adam, grid, block, 0, h->stream, n, h->eta, f1, f2, h->theta, h->grad, h->state[0], h->state[1]);
      break;
    }
    case KG_SV_ADABELIEF: {
      h->evals++;
      const float f2 = 1.0f / (1.0f - std::pow(0.999f, (float)h->evals));
      const float f1 = 1.0f / (1.0f - std::pow(0.9f, (float)h->evals));
      hipLaunchKernelGGL(k_sv_adabelief, grid, block, 0, h->stream, n, h->eta, f1, f2, h->theta, h->grad, h->state[0],
                         h->state[1]);
      break;
    }
    case KG_SV_MADGRAD:
      hipLaunchKernelGGL(k_sv_madgrad, grid, block, 0, h->stream, n, h->eta, h->theta, h->grad, h->state[0], h->state[1],
                         h->state[2]);
      h->evals++;
      break;
    case KG_SV_RMSPROP:
      hipLaunchKernelGGL(k_sv_rmsprop, grid, block, 0, h->stream, n, h->eta, h->theta, h->grad, h->state[0], h->state[1]);
      h->evals++;
      break;
    default:
      hipLaunchKernelGGL(k_sv_adagrad, grid, block, 0, h->stream, n, h->eta, h->theta, h->grad, h->state[0]);
      h->evals++;
      break;
  }
  KG_HIP(hipGetLastError());
  return 0;
}

struct SvField {
  float *ptr = nullptr;
  size_t count = 0;
};

bool sv_field(kg_supervisor_s *h, const std::string &n, SvField &f) {
  if (n == "hyperparameters") return f = {h->theta, h->nh}, true;
  if (n == "gradient") return f = {h->grad, h->nh}, true;
  if (n == "training_input") return f = {h->trainX, h->NB[0] * h->IC}, true;
  if (n == "training_solution") return f = {h->sol, h->NB[0] * h->OC}, true;
  for (size_t i = 0; i < h->stateNames.size(); i++)
    if (n == h->stateNames[i]) return f = {h->state[i], h->nh}, true;
  const size_t c = n.find(':');
  if (c == std::string::npos) return false;
  const std::string base = n.substr(0, c);
  char *end = nullptr;
  const unsigned long l = strtoul(n.c_str() + c + 1, &end, 10);
  if (end == n.c_str() + c + 1 || *end || l >= h->L.size()) return false;
  if (base == "output" || base == "inference_output") {
    const int p = base == "output" ? 0 : h->pipes - 1;
    float *ptr = l == 0 ? const_cast<float *>(h->in[p]) : h->out[p][l];
    if (!ptr) return false;
    return f = {ptr, h->NB[p] * h->L[l].oc}, true;
  }
  if (base == "output_gradient" && h->G[l]) return f = {h->G[l], h->NB[0] * h->L[l].oc}, true;
  return false;
}

}  // namespace

extern "C" {

int kg_supervisor_destroy(kg_supervisor_t h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  std::vector<void *> ptrs = {h->theta, h->grad, h->state[0], h->state[1], h->state[2], h->trainX, h->sol, h->G0,
                              h->ws, h->bpart, h->lpart, h->lossDev, h->scale, h->shift, h->mask};
  for (int p = 0; p < 2; p++)
    for (float *q : h->out[p]) ptrs.push_back(q);
  for (float *q : h->G) ptrs.push_back(q);
  for (void *p : ptrs)
    if (p) dev_release(p);
  if (h->lossHost) host_release(h->lossHost);
  if (h->e0) (void)hipEventDestroy(h->e0);
  if (h->e1) (void)hipEventDestroy(h->e1);
  if (h->stream) stream_release(h->stream);
  delete h;
  return 0;
}

int kg_supervisor_create(const kg_supervisor_config *c, kg_supervisor_t *out) {
  KG_CHECK(c && out, "supervisor: null argument");
  const size_t LIM = (size_t)1 << 31;
  KG_CHECK(c->input_size >= 1 && c->input_size < LIM, "supervisor: input_size must be in [1, 2^31)");
  KG_CHECK(c->solution_size >= 1 && c->solution_size < LIM, "supervisor: solution_size must be in [1, 2^31)");
  KG_CHECK(c->training_batch_size >= 1 && c->training_batch_size < LIM, "supervisor: training_batch_size must be in [1, 2^31)");
  KG_CHECK(c->inference_batch_size >= 1 && c->inference_batch_size < LIM, "supervisor: inference_batch_size must be in [1, 2^31)");
  KG_CHECK(c->layer_count >= 1 && c->layers, "supervisor: no layers given");
  KG_CHECK(c->optimizer >= KG_SV_ADAM && c->optimizer <= KG_SV_ADAGRAD, "supervisor: unknown optimizer");
  KG_CHECK(c->loss == KG_SV_MEAN_SQUARED_ERROR || c->loss == KG_SV_DIRECT_GRADIENT, "supervisor: unknown loss");
  std::vector<Layer> L(1);
  L[0].oc = c->input_size;
  size_t nh = 0, lastLinear = 0;
  for (size_t i = 0; i < c->layer_count; i++) {
    const kg_supervisor_layer &s = c->layers[i];
    Layer ly;
    ly.ic = L.back().oc;
    if (s.type == KG_SV_LINEAR) {
      KG_CHECK(s.output_channels >= 1 && s.output_channels < LIM,
               "supervisor: layer " + std::to_string(i + 1) + ": output_channels must be in [1, 2^31)");
      ly.type = KG_SV_LINEAR, ly.oc = s.output_channels, ly.woff = nh;
      nh += ly.ic * ly.oc + ly.oc;
      lastLinear = i + 1;
    } else if (s.type == KG_SV_ACTIVATION) {
      KG_CHECK(s.function >= KG_SV_TANH && s.function <= KG_SV_SOFTMAX,
               "supervisor: layer " + std::to_string(i + 1) + ": unknown activation function");
      ly.type = KG_SV_ACTIVATION, ly.fn = s.function, ly.alpha = s.alpha, ly.beta = s.beta, ly.oc = ly.ic;
    } else {
      KG_CHECK(false, "supervisor: layer " + std::to_string(i + 1) + ": unknown layer type");
    }
    L.push_back(ly);
  }
  KG_CHECK(lastLinear >= 1, "supervisor: the network has no Linear layer");
  KG_CHECK(L.back().oc == c->solution_size, "supervisor: the last layer's width (" + std::to_string(L.back().oc) +
                                                ") is not solution_size (" + std::to_string(c->solution_size) + ")");
  KG_CHECK(nh < ((size_t)1 << 40), "supervisor: more than 2^40 hyperparameters");
  if (c->output_mask)
    for (size_t j = 0; j < c->solution_size; j++)
      KG_CHECK(c->output_mask[j] >= KG_SV_IDENTITY && c->output_mask[j] <= KG_SV_SIGMOID, "supervisor: unknown output mask");
  {
    Layer ol;
    ol.type = KG_SV_ACTIVATION, ol.ic = ol.oc = c->solution_size;
    L.push_back(ol);
  }
  KG_HIP(hipSetDevice(c->device));
  auto *h = new kg_supervisor_s();
  struct Guard {
    kg_supervisor_s *h;
    ~Guard() {
      if (h) kg_supervisor_destroy(h);
    }
  } guard{h};
  h->device = c->device, h->IC = c->input_size, h->OC = c->solution_size;
  h->NB[0] = c->training_batch_size, h->NB[1] = c->inference_batch_size;
  h->pipes = h->NB[0] == h->NB[1] ? 1 : 2;
  h->nh = nh, h->optimizer = c->optimizer, h->loss = c->loss, h->eta = c->learning_rate;
  h->l2 = c->l2_enabled ? 1 : 0, h->l2imp = c->l2_importance;
  // the split of each weight gradient over the batch: enough workgroups to
  // fill the device (about two per CU), at least 256 rows each
  const size_t B = h->NB[0];
  size_t wsFloats = 0;
  for (auto &ly : L) {
    if (&ly == &L[0] || ly.type != KG_SV_LINEAR) continue;
    const size_t tiles = ((ly.oc + BM - 1) / BM) * ((ly.ic + BM - 1) / BM);
    size_t s = std::min((512 + tiles - 1) / tiles, (B + 255) / 256);
    s = std::max<size_t>(s, 1);
    const size_t chunk = ((B + s - 1) / s + BK - 1) / BK * BK;
    ly.chunk = (int)chunk, ly.splits = (int)((B + chunk - 1) / chunk);
    if (ly.splits > 1) wsFloats = std::max(wsFloats, (size_t)ly.splits * ly.oc * ly.ic);
  }
  h->L = L;
  h->biasSlabs = (int)std::min<size_t>((B + 63) / 64, 256);
  h->biasRows = (int)((B + h->biasSlabs - 1) / h->biasSlabs);
  h->biasSlabs = (int)((B + h->biasRows - 1) / h->biasRows);
  static const std::vector<std::vector<std::string>> names = {{"first_moment", "second_moment"},
                                                              {"first_moment", "second_central_moment"},
                                                              {"s", "v", "z"},
                                                              {"r", "v"},
                                                              {"s"}};
  h->stateNames = names[c->optimizer];
  KG_HIP(stream_acquire(&h->stream));
  KG_HIP(hipEventCreate(&h->e0));
  KG_HIP(hipEventCreate(&h->e1));
  auto alloc = [&](float **p, size_t n) -> int {
    KG_HIP(dev_alloc(p, std::max<size_t>(n, 1) * sizeof(float)));
    return zero_fill_async(*p, std::max<size_t>(n, 1) * sizeof(float));
  };
  if (alloc(&h->theta, nh) || alloc(&h->grad, nh)) return 1;
  for (size_t i = 0; i < h->stateNames.size(); i++)
    if (alloc(&h->state[i], nh)) return 1;
  if (alloc(&h->trainX, B * h->IC) || alloc(&h->sol, B * h->OC) || alloc(&h->G0, B * h->OC)) return 1;
  size_t maxOc = 1;
  for (int p = 0; p < h->pipes; p++) {
    h->out[p].assign(L.size(), nullptr);
    for (size_t l = 0; l < L.size(); l++)
      if (alloc(&h->out[p][l], h->NB[p] * L[l].oc)) return 1;
  }
  h->G.assign(L.size(), nullptr);
  for (size_t l = 1; l + 1 < L.size(); l++) {
    maxOc = std::max(maxOc, L[l].oc);
    if (alloc(&h->G[l], B * L[l].oc)) return 1;
  }
  if (alloc(&h->ws, wsFloats) || alloc(&h->bpart, (size_t)h->biasSlabs * maxOc) || alloc(&h->lpart, LOSS_BLOCKS) ||
      alloc(&h->lossDev, 1))
    return 1;
  KG_HIP(host_alloc(&h->lossHost, sizeof(float), hipHostMallocDefault));
  if (c->output_scale) {
    if (alloc(&h->scale, h->OC)) return 1;
    KG_HIP(hipMemcpy(h->scale, c->output_scale, h->OC * 4, hipMemcpyHostToDevice));
  }
  if (c->output_shift) {
    if (alloc(&h->shift, h->OC)) return 1;
    KG_HIP(hipMemcpy(h->shift, c->output_shift, h->OC * 4, hipMemcpyHostToDevice));
  }
  if (c->output_mask) {
    KG_HIP(dev_alloc(&h->mask, h->OC * sizeof(int)));
    KG_HIP(hipMemcpy(h->mask, c->output_mask, h->OC * sizeof(int), hipMemcpyHostToDevice));
  }
  KG_HIP(hipStreamSynchronize(nullptr));
  guard.h = nullptr;
  *out = h;
  return 0;
}

int kg_supervisor_hyperparameter_count(kg_supervisor_t h, size_t *n) {
  KG_CHECK(h && n, "supervisor: null argument");
  *n = h->nh;
  return 0;
}

int kg_supervisor_set_training_data(kg_supervisor_t h, const float *X, const float *S) {
  KG_CHECK(h && X && S, "supervisor: null argument");
  KG_HIP(hipSetDevice(h->device));
  KG_HIP(hipMemcpyAsync(h->trainX, X, h->NB[0] * h->IC * 4, hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipMemcpyAsync(h->sol, S, h->NB[0] * h->OC * 4, hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->haveData = true;
  return 0;
}

int kg_supervisor_train(kg_supervisor_t h, size_t steps, float *loss) {
  KG_CHECK(h, "supervisor: null argument");
  KG_CHECK(h->haveData, "supervisor: no training data set (kg_supervisor_set_training_data)");
  KG_HIP(hipSetDevice(h->device));
  const bool mse = h->loss == KG_SV_MEAN_SQUARED_ERROR;
  if (!mse)
    KG_CHECK(h->forwarded, "Direct Gradient: there has been no forward pass of 'Training Batch Size' rows whose "
                           "activations the gradients could be propagated through.\n");
  const long long n = (long long)h->NB[0] * h->OC;
  const int last = (int)h->L.size() - 1;
  for (size_t s = 0; s < steps; s++) {
    if (mse) {
      if (sv_forward(h, 0, h->trainX)) return 1;
      {
        SvStage st(h, "other");
        const bool final_ = s + 1 == steps;
        const unsigned lb = std::min<unsigned>(sv_blocks(n), LOSS_BLOCKS);
        hipLaunchKernelGGL(k_sv_mse, dim3(lb), dim3(256), 0, h->stream, n, h->sol, h->out[0][last], h->G0,
                           final_ ? h->lpart : (float *)nullptr);
        if (final_)
          hipLaunchKernelGGL(k_sv_loss, dim3(1), dim3(256), 0, h->stream, (int)lb, h->lpart, (float)h->NB[0], h->lossDev);
      }
      if (sv_backward(h, h->G0)) return 1;
    } else {
      if (sv_backward(h, h->sol)) return 1;
    }
    if (sv_optimize(h)) return 1;
  }
  if (mse && steps > 0) {
    KG_HIP(hipMemcpyAsync(h->lossHost, h->lossDev, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    h->currentLoss = *h->lossHost;
    if (loss) *loss = h->currentLoss;
  } else {
    KG_HIP(hipStreamSynchronize(h->stream));
  }
  return 0;
}

int kg_supervisor_forward(kg_supervisor_t h, const float *X, size_t rows, float *out) {
  KG_CHECK(h && X && out, "supervisor: null argument");
  // the last matching batch size, as NeuralNetwork::getBatchSizeIdx picks it
  int p = -1;
  if (rows == h->NB[0]) p = 0;
  if (rows == h->NB[1]) p = h->pipes - 1;
  if (p < 0) {
    char b[160];
    snprintf(b, sizeof(b), "Batch size (%lu) of input is not within the configured batch sizes of the neural network..\n",
             (unsigned long)rows);
    set_error(b);
    return 1;
  }
  KG_HIP(hipSetDevice(h->device));
  KG_HIP(hipMemcpyAsync(h->out[p][0], X, rows * h->IC * 4, hipMemcpyHostToDevice, h->stream));
  if (sv_forward(h, p, h->out[p][0])) return 1;
  KG_HIP(hipMemcpyAsync(out, h->out[p].back(), rows * h->OC * 4, hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_supervisor_backward_direct(kg_supervisor_t h, const float *G) {
  KG_CHECK(h && G, "supervisor: null argument");
  KG_CHECK(h->forwarded, "Direct Gradient: there has been no forward pass of 'Training Batch Size' rows whose "
                         "activations the gradients could be propagated through.\n");
  KG_HIP(hipSetDevice(h->device));
  KG_HIP(hipMemcpyAsync(h->G0, G, h->NB[0] * h->OC * 4, hipMemcpyHostToDevice, h->stream));
  if (sv_backward(h, h->G0)) return 1;
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_supervisor_field_size(kg_supervisor_t h, const char *name, size_t *elem_bytes, size_t *count) {
  KG_CHECK(h && name && elem_bytes && count, "supervisor: null argument");
  SvField f;
  KG_CHECK(sv_field(h, name, f), std::string("supervisor: unknown field '") + name + "'");
  *elem_bytes = sizeof(float), *count = f.count;
  return 0;
}

int kg_supervisor_get_field(kg_supervisor_t h, const char *name, void *dst, size_t bytes) {
  KG_CHECK(h && name && dst, "supervisor: null argument");
  SvField f;
  KG_CHECK(sv_field(h, name, f), std::string("supervisor: unknown field '") + name + "'");
  KG_CHECK(bytes <= f.count * sizeof(float), "supervisor: field read exceeds its size");
  KG_HIP(hipSetDevice(h->device));
  KG_HIP(hipMemcpyAsync(dst, f.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_supervisor_set_field(kg_supervisor_t h, const char *name, const void *src, size_t bytes) {
  KG_CHECK(h && name && src, "supervisor: null argument");
  SvField f;
  KG_CHECK(sv_field(h, name, f), std::string("supervisor: unknown field '") + name + "'");
  KG_CHECK(bytes <= f.count * sizeof(float), "supervisor: field write exceeds its size");
  KG_HIP(hipSetDevice(h->device));
  KG_HIP(hipMemcpyAsync(f.ptr, src, bytes, hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  if (!strcmp(name, "training_input") || !strcmp(name, "training_solution")) h->haveData = true;
  return 0;
}

int kg_supervisor_get_scalar(kg_supervisor_t h, const char *name, double *value) {
  KG_CHECK(h && name && value, "supervisor: null argument");
  const std::string n = name;
  if (n == "learning_rate") return *value = h->eta, 0;
  if (n == "current_loss") return *value = h->currentLoss, 0;
  if (n == "beta1_pow") return *value = h->b1p, 0;
  if (n == "beta2_pow") return *value = h->b2p, 0;
  if (n == "model_evaluation_count") return *value = (double)h->evals, 0;
  if (n == "layer_count") return *value = (double)h->L.size(), 0;
  if (n == "tile") return *value = BM, 0;
  if (n == "k_step") return *value = BK, 0;
  const size_t c = n.find(':');
  if (c != std::string::npos) {
    const unsigned long l = strtoul(n.c_str() + c + 1, nullptr, 10);
    if (l >= 1 && l + 1 < h->L.size() && h->L[l].type == KG_SV_LINEAR) {
      if (n.compare(0, c, "weight_gradient_splits") == 0) return *value = h->L[l].splits, 0;
      if (n.compare(0, c, "weight_gradient_chunk") == 0) return *value = h->L[l].chunk, 0;
    }
  }
  set_error(std::string("supervisor: unknown scalar '") + name + "'");
  return 1;
}

int kg_supervisor_set_scalar(kg_supervisor_t h, const char *name, double value) {
  KG_CHECK(h && name, "supervisor: null argument");
  const std::string n = name;
  if (n == "learning_rate") return h->eta = (float)value, 0;
  if (n == "beta1_pow") return h->b1p = (float)value, 0;
  if (n == "beta2_pow") return h->b2p = (float)value, 0;
  if (n == "model_evaluation_count") return h->evals = (size_t)value, 0;
  set_error("supervisor: scalar '" + n + "' is not settable");
  return 1;
}

int kg_supervisor_synchronize(kg_supervisor_t h) {
  KG_CHECK(h, "supervisor: null argument");
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_supervisor_profile(kg_supervisor_t h, int enable) {
  KG_CHECK(h, "supervisor: null argument");
  KG_HIP(hipStreamSynchronize(h->stream));
  h->prof = enable ? 1 : 0;
  h->totals.clear();
  return 0;
}

int kg_supervisor_profile_read(kg_supervisor_t h, const char *stage, double *ms_total, size_t *count) {
  KG_CHECK(h && stage && ms_total && count, "supervisor: null argument");
  auto it = h->totals.find(stage);
  *ms_total = it == h->totals.end() ? 0.0 : it->second.first;
  *count = it == h->totals.end() ? 0 : it->second.second;
  if (it != h->totals.end()) h->totals.erase(it);
  return 0;
}

}  // extern "C"
