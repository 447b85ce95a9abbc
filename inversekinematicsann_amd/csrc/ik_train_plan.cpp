// ik_train_plan.cpp -- see ik_train_plan.h.
#include "ik_train_plan.h"

#include <cmath>

#include "../../include/ikhip.h"

namespace ikhip {

namespace {
// One block carved part by part, every part a multiple of 64 floats.
struct Carve {
  size_t total = 0;
  size_t add(size_t n) {
    const size_t at = total;
    total += (n + 63) / 64 * 64;
    return at;
  }
};
}  // namespace

AdamDev train_adam(double lr, double beta1, double beta2, double eps, int64_t t) {
  const double a =
      lr * std::sqrt(1.0 - std::pow(beta2, (double)t)) / (1.0 - std::pow(beta1, (double)t));
  return {beta1, 1.0 - beta1, beta2, 1.0 - beta2, (float)eps, (float)a};
}

TrainStateLayout train_state_layout(int n_layers, const int32_t *dims, int max_batch) {
  TrainStateLayout L = {};
  L.widest = 1;
  for (int l = 0; l <= n_layers; ++l) L.widest = dims[l] > L.widest ? dims[l] : L.widest;
  Carve cv;
  for (int l = 0; l < n_layers; ++l) {
    const size_t kn = (size_t)dims[l] * dims[l + 1], n = (size_t)dims[l + 1];
    L.W[l] = cv.add(kn), L.mW[l] = cv.add(kn), L.vW[l] = cv.add(kn), L.gW[l] = cv.add(kn);
    L.b[l] = cv.add(n), L.mb[l] = cv.add(n), L.vb[l] = cv.add(n), L.gb[l] = cv.add(n);
  }
  for (int l = 0; l <= n_layers; ++l) L.A[l] = cv.add((size_t)max_batch * dims[l]);
  L.y = cv.add((size_t)max_batch * dims[n_layers]);
  L.dZ[0] = cv.add((size_t)max_batch * L.widest), L.dZ[1] = cv.add((size_t)max_batch * L.widest);
  L.total = cv.total;
  return L;
}

TrainDataLayout train_data_layout(int64_t n_train, int64_t n_val, int d0, int dL) {
  TrainDataLayout D;
  Carve cv;
  D.X = cv.add((size_t)n_train * d0), D.Xs = cv.add((size_t)n_train * d0);
  D.Y = cv.add((size_t)n_train * dL), D.Ys = cv.add((size_t)n_train * dL);
  D.Xv = cv.add((size_t)n_val * d0), D.Yv = cv.add((size_t)n_val * dL);
  D.perm = cv.add((size_t)n_train);
  D.total = cv.total;
  return D;
}

TrainEpoch train_epoch(int64_t n_train, int64_t n_val, int batch, int max_batch) {
  return {n_train, n_val, batch, max_batch, (n_train + batch - 1) / batch,
          (n_val + max_batch - 1) / max_batch};
}

void train_epoch_losses(const TrainEpoch &e, int dL, const double *sums, double *train_loss,
                        double *val_loss) {
  double acc = 0.0;
  for (int64_t s = 0; s < e.steps; ++s) {
    const double rows = (double)e.step_rows(s);
    acc += sums[s] / (rows * (double)dL) * rows;
  }
  *train_loss = acc / (double)e.n_train;
  double vs = 0.0;
  for (int64_t v = 0; v < e.vchunks; ++v) vs += sums[e.steps + v];
  *val_loss = e.n_val > 0 ? vs / ((double)e.n_val * (double)dL) : std::nan("");
}

std::string train_begin_refusal(int n_layers, const int32_t *dims, const int32_t *acts,
                                const float *const *W, const float *const *b, int max_batch,
                                double lr, double beta1, double beta2, double eps) {
  if (!dims || !acts || !W || !b) return "NULL argument";
  if (n_layers < 1 || n_layers > kTrainMaxLayers)
    return "n_layers must be 1.." + std::to_string(kTrainMaxLayers);
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > kTrainMaxWidth)
      return "dims[" + std::to_string(l) + "] must be 1.." + std::to_string(kTrainMaxWidth);
  for (int l = 0; l < n_layers; ++l) {
    if (acts[l] < IK_ACT_LINEAR || acts[l] > IK_ACT_SIGMOID) return "unknown activation";
    if (!W[l] || !b[l]) return "NULL layer weights";
  }
  if (max_batch < 1 || max_batch > kTrainMaxBatch)
    return "max_batch must be 1.." + std::to_string(kTrainMaxBatch);
  if (!(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) ||
      !(eps >= 0.0) || !std::isfinite(lr) || !std::isfinite(eps))
    return "bad Adam parameters";
  return "";
}

std::string train_data_refusal(int64_t n_train, int64_t n_val) {
  return n_train < 1 || n_train > INT32_MAX || n_val < 0 || n_val > INT32_MAX ? "bad args" : "";
}

std::string train_epoch_refusal(const int32_t *perm, int64_t n_train, int batch, int max_batch) {
  if (batch < 1 || batch > max_batch)
    return "batch " + std::to_string(batch) + " outside 1..max_batch " + std::to_string(max_batch);
  if (perm)
    for (int64_t i = 0; i < n_train; ++i)
      if (perm[i] < 0 || perm[i] >= n_train)
        return "perm[" + std::to_string(i) + "] = " + std::to_string(perm[i]) + " outside 0.." +
               std::to_string(n_train - 1);
  return "";
}

std::string train_set_loss_refusal(bool begun, int d0, int dL, double mse_weight,
                                   double fk_weight, const double *x_mean, const double *x_scale,
                                   const double *y_mean, const double *y_scale) {
  if (!begun) return "before ik_ann_train_begin";
  if (!std::isfinite(mse_weight) || !std::isfinite(fk_weight) || mse_weight < 0.0 ||
      fk_weight < 0.0)
    return "the weights must be finite and not negative";
  if (mse_weight == 0.0 && fk_weight == 0.0) return "both weights are 0";
  if (!(fk_weight > 0.0)) return "";
  if (d0 != 3 || dL != 4)
    return "the fk term needs 3 inputs and 4 outputs, the network has " + std::to_string(d0) +
           " and " + std::to_string(dL);
  if (!x_mean || !x_scale || !y_mean || !y_scale) return "NULL scaler array";
  const double *arr[4] = {x_mean, x_scale, y_mean, y_scale};
  const char *name[4] = {"x_mean", "x_scale", "y_mean", "y_scale"};
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < (k < 2 ? 3 : 4); ++i) {
      if (!std::isfinite(arr[k][i]))
        return std::string(name[k]) + "[" + std::to_string(i) + "] is not finite";
      if ((k & 1) && arr[k][i] == 0.0)
        return std::string(name[k]) + "[" + std::to_string(i) + "] is 0";
    }
  return "";
}

double train_dz_mse_factor(double mse_weight, int rows, int dL) {
  return mse_weight * 2.0 / ((double)rows * (double)dL);
}

double train_dz_fk_factor(double fk_weight, int rows) { return fk_weight * 2.0 / (double)rows; }

double train_total_loss(double mse_weight, double fk_weight, double mse, double fk) {
  const double m = mse_weight * mse;
  return fk_weight > 0.0 ? m + fk_weight * fk : m;
}

void train_epoch_fk(const TrainEpoch &e, const double *sums, double *train_fk, double *val_fk) {
  double acc = 0.0;
  for (int64_t s = 0; s < e.steps; ++s) {
    const double rows = (double)e.step_rows(s);
    acc += sums[s] / rows * rows;
  }
  *train_fk = acc / (double)e.n_train;
  double vs = 0.0;
  for (int64_t v = 0; v < e.vchunks; ++v) vs += sums[e.steps + v];
  *val_fk = e.n_val > 0 ? vs / (double)e.n_val : std::nan("");
}

}  // namespace ikhip
