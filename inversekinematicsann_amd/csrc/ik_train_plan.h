// ik_train_plan.h -- the host arithmetic of the training calls (ik_train_api.cpp):
// the caps, the layouts of the two device blocks, an epoch's steps and validation
// chunks and what its losses are, Adam's step size, and the arguments the calls
// refuse.  Plain C++, no HIP header, no state: tested on the CPU
// (tests/test_train_plan_cpu.py, tests/host/train_plan_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace ikhip {

constexpr int kTrainMaxLayers = 24;
constexpr int kTrainMaxWidth = 1024;
constexpr int kTrainMaxBatch = 4096;

// What the weight-gradient kernels' Adam epilogue takes (ik_train.hip adam_update).
struct AdamDev {
  double b1, omb1, b2, omb2;  // beta, 1 - beta
  float eps, alpha;           // epsilon, alpha_t
};
// Keras Adam's step size at step t (1-based): alpha_t = lr sqrt(1 - beta2^t) /
// (1 - beta1^t) in float64, then rounded.
AdamDev train_adam(double lr, double beta1, double beta2, double eps, int64_t t);

// The state block (ik_ann_train_begin): offsets in floats, every part a multiple of
// 64 floats, in this order -- per layer W, mW, vW, gW (dims[l] x dims[l + 1] each)
// and b, mb, vb, gb (dims[l + 1] each); then A[0..n_layers] (max_batch x dims[l]),
// y (max_batch x dims[n_layers]) and dZ[0], dZ[1] (max_batch x widest each).
struct TrainStateLayout {
  size_t W[kTrainMaxLayers], mW[kTrainMaxLayers], vW[kTrainMaxLayers], gW[kTrainMaxLayers];
  size_t b[kTrainMaxLayers], mb[kTrainMaxLayers], vb[kTrainMaxLayers], gb[kTrainMaxLayers];
  size_t A[kTrainMaxLayers + 1], y, dZ[2];
  int widest;    // the largest of dims[0..n_layers]
  size_t total;  // floats
};
TrainStateLayout train_state_layout(int n_layers, const int32_t *dims, int max_batch);

// The data block (ik_ann_train_data): offsets in floats of X, Xs (n_train x d0), Y,
// Ys (n_train x dL), Xv (n_val x d0), Yv (n_val x dL) and perm (n_train int32), in
// this order, each part a multiple of 64 floats.
struct TrainDataLayout {
  size_t X, Xs, Y, Ys, Xv, Yv, perm, total;
};
TrainDataLayout train_data_layout(int64_t n_train, int64_t n_val, int d0, int dL);

// One epoch (ik_ann_train_epoch): the training rows in steps of `batch`, then the
// validation rows in chunks of `max_batch`; the last of each may be short.  Loss
// slot s is step s's, slot steps + v chunk v's.
struct TrainEpoch {
  int64_t n_train, n_val;
  int batch, max_batch;
  int64_t steps, vchunks;
  int64_t slots() const { return steps + vchunks; }
  int64_t step_row(int64_t s) const { return s * batch; }
  int step_rows(int64_t s) const { return (int)(n_train - s * batch < batch ? n_train - s * batch : batch); }
  int64_t chunk_row(int64_t v) const { return v * max_batch; }
  int chunk_rows(int64_t v) const {
    return (int)(n_val - v * max_batch < max_batch ? n_val - v * max_batch : max_batch);
  }
};
TrainEpoch train_epoch(int64_t n_train, int64_t n_val, int batch, int max_batch);
// From the slots' sums of squared errors: Keras' running mean of the steps' losses
// weighted by their rows, and the mean over the validation rows (NaN without any).
void train_epoch_losses(const TrainEpoch &e, int dL, const double *sums, double *train_loss,
                        double *val_loss);

// The refusals of the three calls: "" when the arguments are fine, else the text
// after "ik_ann_train_...: ".
std::string train_begin_refusal(int n_layers, const int32_t *dims, const int32_t *acts,
                                const float *const *W, const float *const *b, int max_batch,
                                double lr, double beta1, double beta2, double eps);
std::string train_data_refusal(int64_t n_train, int64_t n_val);
std::string train_epoch_refusal(const int32_t *perm, int64_t n_train, int batch, int max_batch);

// ---- the loss (ik_ann_train_set_loss): mse_weight * mse + fk_weight * fk ----------
// The scalers the forward-kinematics term decodes a row with (ik_train_fk_row.h):
// position = x * xs + xm, theta = a * ys + ym.
struct TrainFkScale {
  double xm[3], xs[3], ym[4], ys[4];
};
// "" or the text after "ik_ann_train_set_loss: ".  begun: a training state exists;
// d0 / dL: its first and last widths.  The scaler arrays are read only when
// fk_weight > 0.
std::string train_set_loss_refusal(bool begun, int d0, int dL, double mse_weight,
                                   double fk_weight, const double *x_mean, const double *x_scale,
                                   const double *y_mean, const double *y_scale);
// The loss kernel's factors of (a_j - y_j) and of (J_j . e) y_scale_j in dZ_L:
// mse_weight 2 / (rows dL) and fk_weight 2 / rows.
double train_dz_mse_factor(double mse_weight, int rows, int dL);
double train_dz_fk_factor(double fk_weight, int rows);
// What the calls return as the loss: mse_weight * mse, plus fk_weight * fk when
// fk_weight > 0 (fk is not read otherwise; weights (1, 0) return mse itself).
double train_total_loss(double mse_weight, double fk_weight, double mse, double fk);
// From the slots' sums of e . e: the steps' fk terms weighted by their rows, and the
// mean over the validation rows (NaN without any).
void train_epoch_fk(const TrainEpoch &e, const double *sums, double *train_fk, double *val_fk);

}  // namespace ikhip
