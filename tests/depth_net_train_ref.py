"""fp64 restatement of the camera-aware DepthNet stage and of its closed-form backward, plain torch on the CPU - the yardstick of the
DepthNet training tests.  Per level, x (N, C, H, W):
    y = conv3x3(x) + b,  xhat = (y - mu) rstd,  z = gamma xhat + beta,  out = relu(z) g[n, c]
with (mu, var) the batch statistics over (N, H, W) (biased variance) or, frozen, the running statistics.  The backward takes the
ReLU mask as an ARGUMENT: the device's gradient is the derivative of the forward the device computed, so a test hands over the
device's own mask and the comparison is free of ReLU decisions at near-zero entries."""
import torch
import torch.nn.functional as F


def forward64(x, w, b, gamma, beta, g, eps, running=None):
    """running = (mean, var): the frozen case.  Returns a dict of fp64 tensors."""
    x, w, b, gamma, beta, g = (t.detach().double().cpu() for t in (x, w, b, gamma, beta, g))
    y = F.conv2d(x, w, b, padding=1)
    if running is None:
        mu, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    else:
        mu, var = (t.detach().double().cpu() for t in running)
    rstd = 1.0 / torch.sqrt(var + eps)
    bc = lambda t: t[None, :, None, None]
    xhat = (y - bc(mu)) * bc(rstd)
    z = bc(gamma) * xhat + bc(beta)
    return dict(x=x, w=w, gamma=gamma, g=g, y=y, mu=mu, var=var, rstd=rstd, xhat=xhat, z=z, out=F.relu(z) * g[:, :, None, None],
                frozen=running is not None)


def backward64(fwd, dout, mask):
    """The closed form: (dx, dW, db, dgamma, dbeta, dg) of sum(out * dout)'s gradient with relu'(z) := mask."""
    x, w, gamma, g, xhat, z, rstd = (fwd[k] for k in ('x', 'w', 'gamma', 'g', 'xhat', 'z', 'rstd'))
    dout, mask = dout.detach().double().cpu(), mask.detach().double().cpu()
    n, c, h, wd = z.shape
    m = n * h * wd
    bc = lambda t: t[None, :, None, None]
    dz = dout * g[:, :, None, None] * mask
    dbeta = dz.sum((0, 2, 3))
    dgamma = (dz * xhat).sum((0, 2, 3))
    dg = (dout * z * mask).sum((2, 3))
    if fwd['frozen']:
        dy = bc(gamma * rstd) * dz
    else:
        dy = bc(gamma * rstd) * (dz - bc(dbeta) / m - xhat * bc(dgamma) / m)
    db = dy.sum((0, 2, 3))
    dx = F.conv2d(dy, w.transpose(0, 1).flip(2, 3), padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.empty_like(w)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', dy, xp[:, :, ky:ky + h, kx:kx + wd])
    return dict(dx=dx, dW=dw, db=db, dgamma=dgamma, dbeta=dbeta, dg=dg, dy=dy)


def running_update(running_mean, running_var, mu, var_biased, m, momentum):
    """One BatchNorm2d training call's buffer update: the running variance takes the UNBIASED variance (x M / (M - 1))."""
    return ((1 - momentum) * running_mean + momentum * mu, (1 - momentum) * running_var + momentum * var_biased * m / (m - 1))


def rel_fro(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))
