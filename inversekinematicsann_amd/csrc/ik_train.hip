// ik_train.hip -- ANN.train_model's fit loop (kinematics/ann.py:27-68) on the GPU:
// forward, MSE loss, backward and the Keras Adam update of a Dense stack.
//
// Restates keras.Model.fit for Input(d0), n x Dense(width, act), Dense(dL) with
// loss='mse' and Adam: per step
//   train_gemm_kernel<FWD>    A_l = act(A_{l-1} W_l + b_l)              (NN, per layer)
//   train_loss_kernel         dZ_L = 2 (A_L - Y) / (rows n_out) act'(A_L), loss sum (float64)
//     (train_loss_fk_kernel in its place once ik_ann_train_set_loss gave the forward-
//      kinematics term a weight: also sum |FK(theta) - p|^2 and its gradient in dZ_L)
//   train_gemm_kernel<DGRAD>  dZ_{l-1} = (dZ_l W_l^T) act'(A_{l-1})      (NT, layers > 1)
//   train_gemm_kernel<WADAM>  [G; g] = [A_{l-1}, 1]^T dZ_l, then Adam on W, b, m, v
//                                                                        (TN, per layer)
// 3 launches per layer and step.  The bias gradient, the column sums of dZ_l, is
// the weight-gradient GEMM's row `in`: A_{l-1} with a column of ones appended (never
// stored: the operand load supplies it).  train_gemm_kernel<WGRAD> stores the
// gradients instead (ik_ann_train_grads).
//
// One GEMM kernel serves the three products: C[M x N] = sum_k Aop[m][k] Bop[k][n]
// with both operands addressed through a row and a column stride, exact fp32 on
// v_mfma_f32_32x32x2_f32.  The training batch is Keras' 32 rows, the layers 500
// wide: a workgroup owns one 32 x 32 output tile (a 32-row panel x a 32-column
// block, so the 32 x 500 forward is 16 workgroups and the 500 x 500 weight
// gradient 256), and its four waves split K between them -- wave w takes the
// 32-deep slices w, w + 4, ... of K -- so a layer's K = 500 is four MFMA chains of
// 64 steps, not one of 250.  The four partial tiles are added through LDS in wave
// order, a fixed order: no floating-point atomics anywhere, and two runs from the
// same state give the same bits.  Loads are guarded (a row, column or k past the
// operand contributes an exact zero), stores are guarded, so any batch, width and
// depth within the caps runs the same code; the next K slice's operands are
// loaded into registers while the current one's MFMAs run.
#include <cstdint>

#include "ik_act.h"
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_train.h"
#include "ik_train_fk_row.h"

namespace ikhip {
namespace train {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Keras Adam (epsilon outside the square root, the bias corrections folded into
// alpha_t on the host).  The moments are stored fp32 but each is evaluated in
// float64 and rounded once: beta m and (1 - beta) g often cancel, and in fp32 the
// roundings of the two products (and of beta itself) would then be several ulp of
// the result.  The weight's own update is fp32.
__device__ __forceinline__ void adam_update(const AdamDev &ad, float g, float *w, float *m,
                                            float *v) {
  const double gd = (double)g;
  const float mn = (float)(ad.b1 * (double)*m + ad.omb1 * gd);
  const float vn = (float)(ad.b2 * (double)*v + ad.omb2 * (gd * gd));
  *m = mn;
  *v = vn;
  *w = *w - ad.alpha * mn / (sqrtf(vn) + ad.eps);
}

enum { EPI_FWD = 0, EPI_DGRAD = 1, EPI_WGRAD = 2, EPI_WADAM = 3 };

struct GemmArgs {
  const float *A;  // Aop[m][k] = A[m sAm + k sAk]
  int sAm, sAk;
  const float *B;  // Bop[k][n] = B[k sBk + n sBn]
  int sBk, sBn;
  int M, N, K;
  int Ma;            // rows of Aop that exist; WGRAD / WADAM: row Ma (M = Ma + 1) is all ones
  float *C;          // Ma x N, row stride N: activations / dZ / W / G
  float *Cb, *mb, *vb;  // WGRAD / WADAM: what row Ma goes to -- b or g (N floats), moments
  const float *aux;  // FWD: bias[N]; DGRAD: the stored outputs the derivative is taken at (M x N)
  int act;
  float *m, *v;  // WADAM: moments, as C
  AdamDev ad;
};

constexpr int kTS = 33;  // LDS row stride of a 32 x 32 tile (odd: conflict-free both ways)

// AK: Aop's k is the unit-stride index (else m); BN: Bop's n is (else k) -- which way
// a wave's 64 lanes run over a 32 x 32 operand slice so that its loads coalesce.
template <bool AK, bool BN, int EPI>
__global__ __launch_bounds__(256) void train_gemm_kernel(GemmArgs g) {
  __shared__ float As[4][32 * kTS];  // [wave][m][k]
  __shared__ float Bs[4][32 * kTS];  // [wave][k][n]
  __shared__ float Rs[4][32 * kTS];  // [wave][m][n] partial tiles
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int nit = (g.K + 127) / 128;
  constexpr bool kOnes = EPI == EPI_WGRAD || EPI == EPI_WADAM;
  float ra[16], rb[16];
  auto load = [&](int it) {
    const int kb = it * 128 + wave * 32;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = i * 64 + lane, lo = e & 31, hi = e >> 5;
      const int am = m0 + (AK ? hi : lo), ak = kb + (AK ? lo : hi);
      ra[i] = (am < g.Ma && ak < g.K) ? g.A[(int64_t)am * g.sAm + (int64_t)ak * g.sAk]
                                      : (kOnes && am == g.Ma && ak < g.K) ? 1.0f : 0.0f;
      const int bk = kb + (BN ? hi : lo), bn = n0 + (BN ? lo : hi);
      rb[i] = (bk < g.K && bn < g.N) ? g.B[(int64_t)bk * g.sBk + (int64_t)bn * g.sBn] : 0.0f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = i * 64 + lane, lo = e & 31, hi = e >> 5;
      As[wave][(AK ? hi : lo) * kTS + (AK ? lo : hi)] = ra[i];
      Bs[wave][(BN ? hi : lo) * kTS + (BN ? lo : hi)] = rb[i];
    }
  };
  f32x16 acc = (f32x16)(0.0f);
  load(0);
  for (int it = 0; it < nit; ++it) {
    store();
    __syncthreads();
    if (it + 1 < nit) load(it + 1);
    // lane (r, h) holds Aop[r][2 s + h] and Bop[2 s + h][r] for MFMA step s
#pragma unroll
    for (int s = 0; s < 16; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wave][r * kTS + 2 * s + h],
                                                 Bs[wave][(2 * s + h) * kTS + r], acc, 0, 0, 0);
    __syncthreads();
  }
  // the wave's partial tile: accumulator q of lane (r, h) is row (q & 3) + 8 (q >> 2) + 4 h,
  // column r
#pragma unroll
  for (int q = 0; q < 16; ++q) Rs[wave][((q & 3) + 8 * (q >> 2) + 4 * h) * kTS + r] = acc[q];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 256 * j, tm = idx >> 5, tn = idx & 31;
    const int m = m0 + tm, n = n0 + tn;
    if (m >= g.M || n >= g.N) continue;
    const int at = tm * kTS + tn;
    const float s = ((Rs[0][at] + Rs[1][at]) + Rs[2][at]) + Rs[3][at];  // wave order, fixed
    const int64_t o = (int64_t)m * g.N + n;
    if (kOnes && m == g.Ma) {  // the ones row: the bias gradient
      if (EPI == EPI_WGRAD)
        g.Cb[n] = s;
      else
        adam_update(g.ad, s, &g.Cb[n], &g.mb[n], &g.vb[n]);
    } else if (EPI == EPI_FWD) {
      g.C[o] = act_apply(g.act, s + g.aux[n]);
    } else if (EPI == EPI_DGRAD) {
      g.C[o] = s * act_deriv(g.act, g.aux[o]);
    } else if (EPI == EPI_WGRAD) {
      g.C[o] = s;
    } else {
      adam_update(g.ad, s, &g.C[o], &g.m[o], &g.v[o]);
    }
  }
}

// dZ_L and the batch's loss sum.  One workgroup: thread t adds elements t, t + 256,
// ... in float64, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void train_loss_kernel(const float *__restrict__ A,
                                                         const float *__restrict__ Y, int total,
                                                         int act, float scale,
                                                         float *__restrict__ dZ,
                                                         double *__restrict__ slot) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < total; i += 256) {
    const float a = A[i];
    const float d = a - Y[i];
    s += (double)d * (double)d;
    if (dZ) dZ[i] = d * scale * act_deriv(act, a);
  }
  sh[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  if (tid == 0) *slot = sh[0];
}

// The loss with the forward-kinematics term (ik_ann_train_set_loss with fk_weight > 0):
// loss = mse_weight mse + fk_weight fk, fk the mean of e . e over the rows,
// e = FK(wrap(theta)) - p (ik_train_fk_row.h).  One workgroup as above; thread t takes
// rows t, t + 256, ..., a row's arithmetic float64 in registers, the robot's constants
// wave-uniform from the constant address space.  dZ_L is evaluated in float64 and
// rounded once.  Two sums, the squared errors' and the e . e's, through the same fixed
// tree: the same bits on every run.
struct LossFkArgs {
  const RobotConstDev *rc;
  const float *A, *X, *Y;  // rows x 4 outputs, rows x 3 inputs, rows x 4 labels
  int rows, act;
  double cm, cf;  // dZ's factors of (a_j - y_j) and of (J_j . e) y_scale_j
  TrainFkScale sc;
  float *dZ;             // rows x 4, or null
  double *slot, *fk_slot;
};

__global__ __launch_bounds__(256) void train_loss_fk_kernel(LossFkArgs g) {
  __shared__ double sh[2][256];
  const RcConst k = (RcConst)g.rc;
  const int tid = threadIdx.x;
  double jc[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) jc[i] = k->jc[i];
  const bool alpha_ok = !k->alpha_bad;
  double sm = 0.0, sf = 0.0;
  for (int r = tid; r < g.rows; r += 256) {
    const float4 a4 = *reinterpret_cast<const float4 *>(g.A + 4 * (int64_t)r);
    const float4 y4 = *reinterpret_cast<const float4 *>(g.Y + 4 * (int64_t)r);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w}, y[4] = {y4.x, y4.y, y4.z, y4.w};
    const float x[3] = {g.X[3 * (int64_t)r], g.X[3 * (int64_t)r + 1], g.X[3 * (int64_t)r + 2]};
    double th[4], s[4], c[4];
    train_fk_angles(g.sc, a, th);
#pragma unroll
    for (int j = 0; j < 4; ++j) sincos_fk(th[j], &s[j], &c[j]);
    const TrainFkRow o = train_fk_row(jc, g.sc, s, c, x, alpha_ok);
    sf += o.ee;
    float dz[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)a[j] - (double)y[j];
      sm += d * d;
      dz[j] = (float)((g.cm * d + g.cf * o.je[j] * g.sc.ys[j]) * (double)act_deriv(g.act, a[j]));
    }
    if (g.dZ)
      *reinterpret_cast<float4 *>(g.dZ + 4 * (int64_t)r) = make_float4(dz[0], dz[1], dz[2], dz[3]);
  }
  sh[0][tid] = sm;
  sh[1][tid] = sf;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      sh[0][tid] += sh[0][tid + w];
      sh[1][tid] += sh[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    *g.slot = sh[0][0];
    *g.fk_slot = sh[1][0];
  }
}

// The epoch's shuffle: row i of the permuted copies is row perm[i] of the data.
__global__ __launch_bounds__(256) void train_gather_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const int32_t *__restrict__ perm,
    int64_t n, int dx, int dy, float *__restrict__ Xs, float *__restrict__ Ys) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int w = dx + dy;
  if (idx >= n * w) return;
  const int64_t row = idx / w;
  const int c = (int)(idx - row * w);
  const int64_t src = perm[row];
  if (c < dx)
    Xs[row * dx + c] = X[src * dx + c];
  else
    Ys[row * dy + (c - dx)] = Y[src * dy + (c - dx)];
}

template <bool AK, bool BN, int EPI>
static void gemm(const char *name, const GemmArgs &g, hipStream_t st) {
  const dim3 grid((unsigned)((g.N + 31) / 32), (unsigned)((g.M + 31) / 32));
  const auto kernel = &train_gemm_kernel<AK, BN, EPI>;
  kt_begin(name, st);
  IK_LAUNCH(kernel, grid, dim3(256), 0, st, g);
  kt_end(st);
}

}  // namespace train

void train_forward(const TrainDev &T, const float *x, int rows, hipStream_t st) {
  using namespace train;
  const float *in = x;
  for (int l = 0; l < T.n_layers; ++l) {
    const int K = T.dims[l], N = T.dims[l + 1];
    GemmArgs g = {};
    g.A = in, g.sAm = K, g.sAk = 1;    // A_{l-1}: rows x K
    g.B = T.W[l], g.sBk = N, g.sBn = 1;  // W_l: K x N
    g.M = g.Ma = rows, g.N = N, g.K = K;
    g.C = T.A[l + 1], g.aux = T.b[l], g.act = T.act[l];
    gemm<true, true, EPI_FWD>("train_fwd_kernel", g, st);
    in = T.A[l + 1];
  }
}

void train_loss(const TrainDev &T, const float *y, int rows, double *slot, bool want_dz,
                hipStream_t st) {
  using namespace train;
  const int L = T.n_layers, n = T.dims[L];
  const float scale = (float)train_dz_mse_factor(T.mse_weight, rows, n);
  kt_begin("train_loss_kernel", st);
  IK_LAUNCH(train_loss_kernel, dim3(1), dim3(256), 0, st, T.A[L], y, rows * n, T.act[L - 1],
            scale, want_dz ? T.dZ[0] : nullptr, slot);
  kt_end(st);
}

void train_loss_fk(const TrainDev &T, const RobotConstDev *rc, const float *x, const float *y,
                   int rows, double *slot, double *fk_slot, bool want_dz, hipStream_t st) {
  using namespace train;
  const int L = T.n_layers;  // dims[0] == 3 and dims[L] == 4 (ik_ann_train_set_loss)
  LossFkArgs g = {};
  g.rc = rc;
  g.A = T.A[L], g.X = x, g.Y = y;
  g.rows = rows, g.act = T.act[L - 1];
  g.cm = train_dz_mse_factor(T.mse_weight, rows, 4);
  g.cf = train_dz_fk_factor(T.fk_weight, rows);
  g.sc = T.fk_scale;
  g.dZ = want_dz ? T.dZ[0] : nullptr;
  g.slot = slot, g.fk_slot = fk_slot;
  kt_begin("train_loss_fk_kernel", st);
  IK_LAUNCH(train_loss_fk_kernel, dim3(1), dim3(256), 0, st, g);
  kt_end(st);
}

void train_backward(const TrainDev &T, const float *x, int rows, bool adam, const AdamDev &ad,
                    hipStream_t st) {
  using namespace train;
  int cur = 0;  // dZ[cur] holds dZ_l
  for (int l = T.n_layers - 1; l >= 0; --l) {
    const int K = T.dims[l], N = T.dims[l + 1];
    const float *prev = l == 0 ? x : T.A[l];  // A_{l-1}: rows x K
    if (l > 0) {
      // dZ_{l-1} = (dZ_l W_l^T) act'(A_{l-1}): rows x K, reducing over N; before W_l moves
      GemmArgs g = {};
      g.A = T.dZ[cur], g.sAm = N, g.sAk = 1;
      g.B = T.W[l], g.sBk = 1, g.sBn = N;  // Bop[k = out][n = in] = W[in][out]
      g.M = g.Ma = rows, g.N = K, g.K = N;
      g.C = T.dZ[cur ^ 1], g.aux = prev, g.act = T.act[l - 1];
      gemm<true, false, EPI_DGRAD>("train_dgrad_kernel", g, st);
    }
    {
      // [G; g] = [A_{l-1}, 1]^T dZ_l: (K + 1) x N, reducing over the rows
      GemmArgs g = {};
      g.A = prev, g.sAm = 1, g.sAk = K;  // Aop[m = in][k = row]
      g.B = T.dZ[cur], g.sBk = N, g.sBn = 1;
      g.Ma = K, g.M = K + 1, g.N = N, g.K = rows;
      g.ad = ad;
      if (adam) {
        g.C = T.W[l], g.m = T.mW[l], g.v = T.vW[l];
        g.Cb = T.b[l], g.mb = T.mb[l], g.vb = T.vb[l];
        gemm<false, true, EPI_WADAM>("train_wgrad_adam_kernel", g, st);
      } else {
        g.C = T.gW[l], g.Cb = T.gb[l];
        gemm<false, true, EPI_WGRAD>("train_wgrad_kernel", g, st);
      }
    }
    cur ^= 1;
  }
}

void train_gather(const TrainDev &T, hipStream_t st) {
  using namespace train;
  const int dx = T.dims[0], dy = T.dims[T.n_layers];
  const int64_t total = T.n_train * (dx + dy);
  kt_begin("train_gather_kernel", st);
  IK_LAUNCH(train_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T.X,
            T.Y, T.perm, T.n_train, dx, dy, T.Xs, T.Ys);
  kt_end(st);
}

}  // namespace ikhip
