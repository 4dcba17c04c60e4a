"""BatchNorm on FROZEN statistics (bn.eval() inside a training backbone), restated in fp64 torch on the CPU from its definition - the
reference of tests/test_cpu_frozen_bn.py and tests/test_gpu_frozen_bn.py.  Tensors are NHWC like the kernels' (channels last).

    rstd = 1 / sqrt(running_var + eps);  s = gamma rstd;  t = beta - running_mean s
    z = relu?(y s + t (+ res))
    g = relu ? dz [z > 0] : dz;  dres = g;  dy = g s;  dbeta = sum g;  dgamma = sum g (y - running_mean) rstd
"""

import torch
import torch.nn.functional as F


def fold(gamma, beta, running_mean, running_var, eps):
    """-> (s, t, rstd) in fp64."""
    rstd = 1.0 / torch.sqrt(running_var.double() + eps)
    s = gamma.double() * rstd
    return s, beta.double() - running_mean.double() * s, rstd


def forward(y, gamma, beta, running_mean, running_var, eps, res=None, relu=True):
    """z (fp64) of the NHWC tensor y."""
    s, t, _ = fold(gamma, beta, running_mean, running_var, eps)
    z = y.double() * s + t
    if res is not None:
        z = z + res.double()
    return z.relu() if relu else z


def backward(dz, z, y, gamma, running_mean, running_var, eps, relu=True):
    """-> (dy, dres, dgamma, dbeta) in fp64 from the gradient dz of z; ``z``: the forward's output (its sign is the ReLU mask)."""
    s, _, rstd = fold(gamma, torch.zeros_like(gamma), running_mean, running_var, eps)
    g = dz.double() * (z.double() > 0) if relu else dz.double()
    C = g.shape[-1]
    xh = (y.double() - running_mean.double()) * rstd
    return g * s, g, (g * xh).reshape(-1, C).sum(0), g.reshape(-1, C).sum(0)


def pool_forward(y, gamma, beta, running_mean, running_var, eps):
    """The stem: max_pool2d(relu(BN_frozen(y)), 3, 2, 1) of the NHWC tensor y -> (p NHWC, the flat winner indices of F.max_pool2d)."""
    z = forward(y, gamma, beta, running_mean, running_var, eps).permute(0, 3, 1, 2)
    p, idx = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    return p.permute(0, 2, 3, 1), idx


def pool_backward(dp, y, gamma, beta, running_mean, running_var, eps):
    """-> (dy, dgamma, dbeta) in fp64 from the gradient dp (NHWC) of the pooled map: the pool's winners (first maximum in scan order, as
    ATen's kernel and sd_bn_relu_pool_fwd) take the gradient, then ``backward``."""
    z = forward(y, gamma, beta, running_mean, running_var, eps)
    zc = z.permute(0, 3, 1, 2)
    _, idx = F.max_pool2d(zc, 3, 2, 1, return_indices=True)
    dzc = torch.zeros_like(zc).flatten(2)
    dzc.scatter_add_(2, idx.flatten(2), dp.double().permute(0, 3, 1, 2).flatten(2))
    dz = dzc.view_as(zc).permute(0, 2, 3, 1)
    dy, _, dgamma, dbeta = backward(dz, z, y, gamma, running_mean, running_var, eps, relu=True)
    return dy, dgamma, dbeta


def unit(h, w, gamma, beta, running_mean, running_var, eps, stride, res=None, relu=True):
    """conv (k x k, padding k // 2, ``stride``) -> frozen BatchNorm (+ res) (+ ReLU) on NHWC fp64 tensors that may require a gradient (autograd
    gives dW, dh, dres, dgamma, dbeta): -> z NHWC."""
    y = F.conv2d(h.permute(0, 3, 1, 2), w, stride=stride, padding=w.shape[-1] // 2).permute(0, 2, 3, 1)
    rstd = 1.0 / torch.sqrt(running_var + eps)
    s = gamma * rstd
    z = y * s + (beta - running_mean * s)
    if res is not None:
        z = z + res
    return z.relu() if relu else z
