"""The training loss with the forward-kinematics term, restated with torch for the
tests (tests/test_train_fk_cpu.py, tests/test_gpu_train_fk.py): autograd does the
derivative, and the chain is written independently of kinematics/refine.py's -- the
product of the four 4 x 4 DH matrices Rz(theta) Tz(d) Tx(a) Rx(alpha) the way
kinematics/forward.py forms them, the effector its translation."""
import math

import numpy as np

# the scalers of the gradient cases
X_SCALER = (np.array([2.5, 0.3, 1.5]), np.array([1.2, 1.8, 1.4]))
Y_SCALER = (np.array([0.2, 0.8, -0.7, 0.1]), np.array([0.9, 0.5, 0.6, 0.8]))


def _torch():
    import torch
    torch.set_num_threads(4)
    return torch


def fk_torch(dh, th):
    """Effector positions (n x 3) of the angle rows th (n x 4, float64 tensor)."""
    torch = _torch()
    dh = np.asarray(dh, np.float64).reshape(4, 4)
    n = th.shape[0]
    T = torch.eye(4, dtype=th.dtype).expand(n, 4, 4)
    for i in range(4):
        c, s = torch.cos(th[:, i]), torch.sin(th[:, i])
        rz = torch.eye(4, dtype=th.dtype).repeat(n, 1, 1)
        rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = c, -s, s, c
        tz = torch.eye(4, dtype=th.dtype)
        tz[2, 3] = float(dh[1, i])
        tx = torch.eye(4, dtype=th.dtype)
        tx[0, 3] = float(dh[2, i])
        ca, sa = math.cos(dh[3, i]), math.sin(dh[3, i])
        rx = torch.eye(4, dtype=th.dtype)
        rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = ca, -sa, sa, ca
        T = T @ (rz @ tz @ tx @ rx)
    return T[:, :3, 3]


def loss_parts(a, x, y, x_scaler, y_scaler, dh):
    """(mse, fk) of the outputs a (a tensor of any float dtype), evaluated in float64
    from them: what the loss kernel does with the network's fp32 outputs."""
    torch = _torch()
    f64 = torch.float64
    a = a.to(f64)
    x = torch.as_tensor(np.asarray(x, np.float64))
    y = torch.as_tensor(np.asarray(y, np.float64))
    xm, xs = (torch.as_tensor(np.asarray(v, np.float64)) for v in x_scaler)
    ym, ys = (torch.as_tensor(np.asarray(v, np.float64)) for v in y_scaler)
    mse = ((a - y) ** 2).sum() / (a.shape[0] * 4)
    e = fk_torch(dh, a * ys + ym) - (x * xs + xm)
    fk = (e * e).sum() / a.shape[0]
    return mse, fk
