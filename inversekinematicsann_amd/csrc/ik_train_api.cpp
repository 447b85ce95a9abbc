// ik_train_api.cpp -- the training calls of the C ABI (ik_ann_train_*, declared in
// include/ikhip.h; kernels: ik_train.hip).  Call bodies only: the layouts of the
// device blocks, the epoch's steps and chunks, the losses, Adam's step size and the
// refused arguments are the host-only ik_train_plan.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "ik_internal.h"
#include "ik_train.h"
#include "ik_train_plan.h"

using namespace ikhip;
using namespace ikapi;

namespace {

void train_free_data(TrainDev *T) {
  if (T->data_block) (void)hipFree(T->data_block);
  T->data_block = nullptr;
  T->X = T->Y = T->Xs = T->Ys = T->Xv = T->Yv = nullptr;
  T->perm = nullptr;
  T->n_train = T->n_val = 0;
}

AdamDev next_adam(const TrainDev *T) {
  return train_adam(T->lr, T->beta1, T->beta2, T->eps, T->t + 1);
}

int train_slots(ik_ctx *c, int64_t want) {
  TrainDev *T = c->train;
  if (want <= T->loss_slots) return IK_OK;
  IK_HIP(hipStreamSynchronize(c->stream));
  if (T->loss) IK_HIP(hipFree(T->loss));
  T->loss = nullptr;
  T->loss_slots = 0;
  // two doubles a slot: with the fk term a slot is {squared errors' sum, fk sum}, so one
  // copy brings both back; without it the sums lie one double apart as they always did
  IK_HIP(hipMalloc(reinterpret_cast<void **>(&T->loss), 2 * (size_t)want * sizeof(double)));
  T->loss_slots = want;
  return IK_OK;
}

// The loss kernel of the rows x (device), labels y, into slot `at`.
void loss_launch(ik_ctx *c, const float *x, const float *y, int rows, int64_t at, bool want_dz) {
  const TrainDev *T = c->train;
  if (T->fk_weight > 0.0)
    train_loss_fk(*T, c->rconst, x, y, rows, T->loss + 2 * at, T->loss + 2 * at + 1, want_dz,
                  c->stream);
  else
    train_loss(*T, y, rows, T->loss + at, want_dz, c->stream);
}

// One batch from host rows: forward, loss, backward (Adam update or gradients out).
int train_batch(ik_ctx *c, const char *who, const float *x, const float *y, int rows, bool adam,
                double *loss) {
  TrainDev *T = c->train;
  if (!T) return fail(IK_E_BADARG, std::string(who) + ": before ik_ann_train_begin");
  if (!x || !y || rows < 1)
    return fail(IK_E_BADARG, std::string(who) + ": NULL rows or rows < 1");
  if (rows > T->max_batch)
    return fail(IK_E_BADARG, std::string(who) + ": " + std::to_string(rows) +
                                 " rows exceed max_batch " + std::to_string(T->max_batch));
  const int d0 = T->dims[0], dL = T->dims[T->n_layers];
  IK_HIP(hipMemcpyAsync(T->A[0], x, (size_t)rows * d0 * sizeof(float), hipMemcpyHostToDevice,
                        c->stream));
  IK_HIP(hipMemcpyAsync(T->y, y, (size_t)rows * dL * sizeof(float), hipMemcpyHostToDevice,
                        c->stream));
  train_forward(*T, T->A[0], rows, c->stream);
  loss_launch(c, T->A[0], T->y, rows, 0, true);
  train_backward(*T, T->A[0], rows, adam, next_adam(T), c->stream);
  IK_HIP(hipGetLastError());
  const bool fk = T->fk_weight > 0.0;
  double sum[2] = {0.0, 0.0};  // {squared errors, fk}
  IK_HIP(hipMemcpyAsync(sum, T->loss, (fk ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  IK_HIP(hipStreamSynchronize(c->stream));
  if (adam) T->t += 1;
  T->last_train_fk = fk ? sum[1] / (double)rows : std::nan("");
  T->last_val_fk = std::nan("");
  if (loss)
    *loss = train_total_loss(T->mse_weight, T->fk_weight, sum[0] / ((double)rows * (double)dL),
                             T->last_train_fk);
  return IK_OK;
}

}  // namespace

namespace ikapi {

void train_release(ik_ctx *c) {
  TrainDev *T = c->train;
  if (!T) return;
  (void)hipStreamSynchronize(c->stream);
  train_free_data(T);
  if (T->loss) (void)hipFree(T->loss);
  if (T->block) (void)hipFree(T->block);
  delete T;
  c->train = nullptr;
}

}  // namespace ikapi

extern "C" {

int ik_ann_train_begin(ik_ctx *c, int n_layers, const int32_t *dims, const int32_t *acts,
                       const float *const *W, const float *const *b, int max_batch, double lr,
                       double beta1, double beta2, double eps) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_begin: NULL argument");
  const std::string why =
      train_begin_refusal(n_layers, dims, acts, W, b, max_batch, lr, beta1, beta2, eps);
  if (!why.empty()) return fail(IK_E_BADARG, "ik_ann_train_begin: " + why);
  int rc = set_dev(c);
  if (rc) return rc;
  train_release(c);  // a second begin starts over
  TrainDev *T = new (std::nothrow) TrainDev;
  if (!T) return fail(IK_E_HIP, "ik_ann_train_begin: out of host memory");
  c->train = T;
  T->n_layers = n_layers;
  T->max_batch = max_batch;
  T->lr = lr, T->beta1 = beta1, T->beta2 = beta2, T->eps = eps;
  for (int l = 0; l <= n_layers; ++l) T->dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) T->act[l] = acts[l];
  const TrainStateLayout L = train_state_layout(n_layers, dims, max_batch);
  auto bail = [&](int code) {
    train_release(c);
    return code;
  };
  if (hipMalloc(&T->block, L.total * sizeof(float)) != hipSuccess) {
    T->block = nullptr;
    (void)hipGetLastError();
    return bail(fail(IK_E_HIP, "ik_ann_train_begin: hipMalloc of the training state failed"));
  }
  float *p = static_cast<float *>(T->block);
  for (int l = 0; l < n_layers; ++l) {
    T->W[l] = p + L.W[l], T->mW[l] = p + L.mW[l], T->vW[l] = p + L.vW[l], T->gW[l] = p + L.gW[l];
    T->b[l] = p + L.b[l], T->mb[l] = p + L.mb[l], T->vb[l] = p + L.vb[l], T->gb[l] = p + L.gb[l];
  }
  for (int l = 0; l <= n_layers; ++l) T->A[l] = p + L.A[l];
  T->y = p + L.y, T->dZ[0] = p + L.dZ[0], T->dZ[1] = p + L.dZ[1];
  if ((rc = train_slots(c, 1))) return bail(rc);
  hipError_t e = hipMemsetAsync(T->block, 0, L.total * sizeof(float), c->stream);
  for (int l = 0; l < n_layers && e == hipSuccess; ++l) {
    e = hipMemcpyAsync(T->W[l], W[l], (size_t)dims[l] * dims[l + 1] * sizeof(float),
                       hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(T->b[l], b[l], (size_t)dims[l + 1] * sizeof(float),
                         hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return bail(fail(IK_E_HIP, std::string("ik_ann_train_begin: ") + hipGetErrorString(e)));
  return IK_OK;
}

int ik_ann_train_set_loss(ik_ctx *c, double mse_weight, double fk_weight, const double *x_mean,
                          const double *x_scale, const double *y_mean, const double *y_scale) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_set_loss: NULL context");
  TrainDev *T = c->train;
  const std::string why =
      train_set_loss_refusal(T != nullptr, T ? T->dims[0] : 0, T ? T->dims[T->n_layers] : 0,
                             mse_weight, fk_weight, x_mean, x_scale, y_mean, y_scale);
  if (!why.empty()) return fail(IK_E_BADARG, "ik_ann_train_set_loss: " + why);
  T->mse_weight = mse_weight, T->fk_weight = fk_weight;
  if (fk_weight > 0.0)
    for (int i = 0; i < 4; ++i) {
      if (i < 3) T->fk_scale.xm[i] = x_mean[i], T->fk_scale.xs[i] = x_scale[i];
      T->fk_scale.ym[i] = y_mean[i], T->fk_scale.ys[i] = y_scale[i];
    }
  T->last_train_fk = T->last_val_fk = std::nan("");
  return IK_OK;
}

int ik_ann_train_fk(ik_ctx *c, double *train_fk, double *val_fk) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_fk: NULL context");
  const TrainDev *T = c->train;
  if (!T) return fail(IK_E_BADARG, "ik_ann_train_fk: before ik_ann_train_begin");
  if (train_fk) *train_fk = T->last_train_fk;
  if (val_fk) *val_fk = T->last_val_fk;
  return IK_OK;
}

int ik_ann_train_data(ik_ctx *c, const float *x, const float *y, int64_t n_train, const float *xv,
                      const float *yv, int64_t n_val) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_data: NULL context");
  TrainDev *T = c->train;
  if (!T) return fail(IK_E_BADARG, "ik_ann_train_data: before ik_ann_train_begin");
  if (!x || !y || !train_data_refusal(n_train, n_val).empty() || (n_val > 0 && (!xv || !yv)))
    return fail(IK_E_BADARG, "ik_ann_train_data: bad args");
  int rc = set_dev(c);
  if (rc) return rc;
  IK_HIP(hipStreamSynchronize(c->stream));
  train_free_data(T);
  const size_t d0 = (size_t)T->dims[0], dL = (size_t)T->dims[T->n_layers];
  const TrainDataLayout D = train_data_layout(n_train, n_val, (int)d0, (int)dL);
  IK_HIP(hipMalloc(&T->data_block, D.total * sizeof(float)));
  float *p = static_cast<float *>(T->data_block);
  T->X = p + D.X, T->Xs = p + D.Xs, T->Y = p + D.Y, T->Ys = p + D.Ys;
  T->Xv = p + D.Xv, T->Yv = p + D.Yv;
  T->perm = reinterpret_cast<int32_t *>(p + D.perm);
  T->n_train = n_train;
  T->n_val = n_val;
  IK_HIP(hipMemcpyAsync(T->X, x, (size_t)n_train * d0 * 4, hipMemcpyHostToDevice, c->stream));
  IK_HIP(hipMemcpyAsync(T->Y, y, (size_t)n_train * dL * 4, hipMemcpyHostToDevice, c->stream));
  if (n_val > 0) {
    IK_HIP(hipMemcpyAsync(T->Xv, xv, (size_t)n_val * d0 * 4, hipMemcpyHostToDevice, c->stream));
    IK_HIP(hipMemcpyAsync(T->Yv, yv, (size_t)n_val * dL * 4, hipMemcpyHostToDevice, c->stream));
  }
  IK_HIP(hipStreamSynchronize(c->stream));
  return IK_OK;
}

int ik_ann_train_grads(ik_ctx *c, const float *x, const float *y, int rows, float *const *dW,
                       float *const *db, double *loss) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_grads: NULL context");
  if (c->train && (!dW || !db)) return fail(IK_E_BADARG, "ik_ann_train_grads: NULL outputs");
  int rc = set_dev(c);
  if (rc) return rc;
  KtScope kts(c);
  if ((rc = train_batch(c, "ik_ann_train_grads", x, y, rows, false, loss))) return rc;
  const TrainDev *T = c->train;
  for (int l = 0; l < T->n_layers; ++l) {
    if (dW[l])
      IK_HIP(hipMemcpyAsync(dW[l], T->gW[l], (size_t)T->dims[l] * T->dims[l + 1] * 4,
                            hipMemcpyDeviceToHost, c->stream));
    if (db[l])
      IK_HIP(hipMemcpyAsync(db[l], T->gb[l], (size_t)T->dims[l + 1] * 4, hipMemcpyDeviceToHost,
                            c->stream));
  }
  IK_HIP(hipStreamSynchronize(c->stream));
  return IK_OK;
}

int ik_ann_train_step(ik_ctx *c, const float *x, const float *y, int rows, double *loss) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_step: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  KtScope kts(c);
  return train_batch(c, "ik_ann_train_step", x, y, rows, true, loss);
}

int ik_ann_train_epoch(ik_ctx *c, const int32_t *perm, int batch, double *train_loss_out,
                       double *val_loss_out) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_epoch: NULL context");
  TrainDev *T = c->train;
  if (!T) return fail(IK_E_BADARG, "ik_ann_train_epoch: before ik_ann_train_begin");
  if (!T->data_block) return fail(IK_E_BADARG, "ik_ann_train_epoch: before ik_ann_train_data");
  const std::string why = train_epoch_refusal(perm, T->n_train, batch, T->max_batch);
  if (!why.empty()) return fail(IK_E_BADARG, "ik_ann_train_epoch: " + why);
  int rc = set_dev(c);
  if (rc) return rc;
  const TrainEpoch ep = train_epoch(T->n_train, T->n_val, batch, T->max_batch);
  if ((rc = train_slots(c, ep.slots()))) return rc;
  KtScope kts(c);
  const size_t d0 = (size_t)T->dims[0], dL = (size_t)T->dims[T->n_layers];
  const float *xs = T->X, *ys = T->Y;
  if (perm) {
    IK_HIP(hipMemcpyAsync(T->perm, perm, (size_t)T->n_train * sizeof(int32_t),
                          hipMemcpyHostToDevice, c->stream));
    train_gather(*T, c->stream);
    xs = T->Xs, ys = T->Ys;
  }
  for (int64_t s = 0; s < ep.steps; ++s) {
    const int64_t r0 = ep.step_row(s);
    const int rows = ep.step_rows(s);
    train_forward(*T, xs + r0 * d0, rows, c->stream);
    loss_launch(c, xs + r0 * d0, ys + r0 * dL, rows, s, true);
    train_backward(*T, xs + r0 * d0, rows, true, next_adam(T), c->stream);
    T->t += 1;
  }
  // the end-of-epoch weights over the validation rows, forward only
  for (int64_t v = 0; v < ep.vchunks; ++v) {
    const int64_t r0 = ep.chunk_row(v);
    const int rows = ep.chunk_rows(v);
    train_forward(*T, T->Xv + r0 * d0, rows, c->stream);
    loss_launch(c, T->Xv + r0 * d0, T->Yv + r0 * dL, rows, ep.steps + v, false);
  }
  IK_HIP(hipGetLastError());
  const bool fk = T->fk_weight > 0.0;
  std::vector<double> sums((size_t)ep.slots() * (fk ? 2 : 1)), fsums;
  IK_HIP(hipMemcpyAsync(sums.data(), T->loss, sums.size() * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  IK_HIP(hipStreamSynchronize(c->stream));
  if (fk) {  // {squared errors, fk} pairs apart
    fsums.resize((size_t)ep.slots());
    for (size_t i = 0; i < fsums.size(); ++i) fsums[i] = sums[2 * i + 1], sums[i] = sums[2 * i];
  }
  double tl, vl;
  train_epoch_losses(ep, (int)dL, sums.data(), &tl, &vl);
  T->last_train_fk = T->last_val_fk = std::nan("");
  if (fk) train_epoch_fk(ep, fsums.data(), &T->last_train_fk, &T->last_val_fk);
  if (train_loss_out)
    *train_loss_out = train_total_loss(T->mse_weight, T->fk_weight, tl, T->last_train_fk);
  if (val_loss_out)
    *val_loss_out = train_total_loss(T->mse_weight, T->fk_weight, vl, T->last_val_fk);
  return IK_OK;
}

int ik_ann_train_get(ik_ctx *c, int what, float *const *W, float *const *b) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_get: NULL context");
  const TrainDev *T = c->train;
  if (!T) return fail(IK_E_BADARG, "ik_ann_train_get: before ik_ann_train_begin");
  if (what < 0 || what > 2 || !W || !b) return fail(IK_E_BADARG, "ik_ann_train_get: bad args");
  int rc = set_dev(c);
  if (rc) return rc;
  float *const *sw = what == 0 ? T->W : what == 1 ? T->mW : T->vW;
  float *const *sb = what == 0 ? T->b : what == 1 ? T->mb : T->vb;
  for (int l = 0; l < T->n_layers; ++l) {
    if (W[l])
      IK_HIP(hipMemcpyAsync(W[l], sw[l], (size_t)T->dims[l] * T->dims[l + 1] * 4,
                            hipMemcpyDeviceToHost, c->stream));
    if (b[l])
      IK_HIP(hipMemcpyAsync(b[l], sb[l], (size_t)T->dims[l + 1] * 4, hipMemcpyDeviceToHost,
                            c->stream));
  }
  IK_HIP(hipStreamSynchronize(c->stream));
  return IK_OK;
}

int ik_ann_train_end(ik_ctx *c) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_train_end: NULL context");
  if (!c->train) return fail(IK_E_BADARG, "ik_ann_train_end: before ik_ann_train_begin");
  int rc = set_dev(c);
  if (rc) return rc;
  train_release(c);
  return IK_OK;
}

}  // extern "C"
