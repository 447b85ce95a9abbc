// ik_train.h -- the training state on the device and the launchers of ik_train.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_train_plan.h"

namespace ikhip {

struct RobotConstDev;  // ik_fk_chain.h

// Training (ik_train.hip): ANN.train_model's Keras fit (kinematics/ann.py:27-68)
// as plain stream launches -- per step one forward GEMM per layer, one loss
// kernel, one data-gradient GEMM per layer after the first, and per layer one
// weight-gradient GEMM (the bias gradient its last row) with the Adam update in its
// epilogue.
// Master weights, moments and gradients are fp32 row-major [in][out] (the Keras
// kernel layout), unpadded; every activation row is dims[l] floats.  The caps,
// AdamDev and the blocks' layouts: ik_train_plan.h.
struct TrainDev {
  int n_layers = 0, max_batch = 0;
  int dims[kTrainMaxLayers + 1] = {};
  int act[kTrainMaxLayers] = {};
  float *W[kTrainMaxLayers] = {}, *b[kTrainMaxLayers] = {};
  float *mW[kTrainMaxLayers] = {}, *mb[kTrainMaxLayers] = {};  // Adam first moments
  float *vW[kTrainMaxLayers] = {}, *vb[kTrainMaxLayers] = {};  // Adam second moments
  float *gW[kTrainMaxLayers] = {}, *gb[kTrainMaxLayers] = {};  // gradients (ik_ann_train_grads)
  float *A[kTrainMaxLayers + 1] = {};  // A[0]: staged inputs; A[l]: layer l's outputs of the batch
  float *y = nullptr;                  // staged targets
  float *dZ[2] = {};                   // max_batch x widest layer, alternating
  // loss-sum slots (one per step / validation chunk): 2 loss_slots doubles -- a double
  // a slot, or with the fk term two, {squared errors' sum, fk sum}
  double *loss = nullptr;
  int64_t loss_slots = 0;
  // the loss (ik_ann_train_set_loss): mse_weight * mse + fk_weight * fk
  double mse_weight = 1.0, fk_weight = 0.0;
  TrainFkScale fk_scale = {};
  double last_train_fk = __builtin_nan(""), last_val_fk = __builtin_nan("");  // ik_ann_train_fk
  void *block = nullptr;               // the allocation the pointers above the slots point into
  double lr = 0, beta1 = 0, beta2 = 0, eps = 0;
  int64_t t = 0;                       // Adam steps taken
  // the data set (ik_ann_train_data): scaled fp32 rows, and their permuted copies
  float *X = nullptr, *Y = nullptr, *Xs = nullptr, *Ys = nullptr, *Xv = nullptr, *Yv = nullptr;
  int32_t *perm = nullptr;
  int64_t n_train = 0, n_val = 0;
  void *data_block = nullptr;
};
// A_l = act(A_{l-1} W_l + b_l) for every layer; x: rows x dims[0] device floats.
void train_forward(const TrainDev &T, const float *x, int rows, hipStream_t st);
// *slot = sum((A_L - y)^2) in float64; with want_dz, dZ[0] = mse_weight 2 (A_L - y) /
// (rows n_out) * act'(A_L).
void train_loss(const TrainDev &T, const float *y, int rows, double *slot, bool want_dz,
                hipStream_t st);
// The loss with the forward-kinematics term (fk_weight > 0; ik_train_fk_row.h): also
// *fk_slot = sum(e . e) over the rows, e = FK(wrap(theta)) - p of the robot rc from the
// outputs A_L and the inputs x (rows x 3, device), and dZ[0] of the weighted sum.
void train_loss_fk(const TrainDev &T, const RobotConstDev *rc, const float *x, const float *y,
                   int rows, double *slot, double *fk_slot, bool want_dz, hipStream_t st);
// The backward pass from dZ[0]: with adam, W / b / m / v are updated in the weight-
// gradient kernels' epilogues; without, the gradients go to gW / gb.
void train_backward(const TrainDev &T, const float *x, int rows, bool adam, const AdamDev &ad,
                    hipStream_t st);
// Xs[i] = X[perm[i]], Ys[i] = Y[perm[i]] over the training rows.
void train_gather(const TrainDev &T, hipStream_t st);

}  // namespace ikhip
