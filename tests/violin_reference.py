"""Float64 restatement of the VIOLIN head's two kernels and their gradients, written from the formulas
(HeroForViolin.get_modularized_video and forward, model/violin.py:30-47, 73-81) - no autograd, no einsum, no library kernel:

  frame pool    s[v,l] = <X[v,l,:], w>  through  s * m + (1 - m) * -1e4
                att = softmax over l,  pooled[v,:] = sum_l att X                    (S, D)
                d att[v,l] = <dpooled[v,:], X[v,l,:]>
                ds = att * (d att - sum_l(att * d att)) * m          (softmax backward, times d mask_logits / ds)
                dX[v,l,:] = att dpooled[v,:] + ds w,   dw = sum_{v,l} ds X

  classifier    z[s] = <h[s,:], w> + b
  tail          term_s = min(softplus(-z), 100) for t = 1, min(softplus(z), 100) for t = 0,  softplus(z) = max(z, 0) + log1p(exp(-|z|))
                loss = mean_s term_s            (= binary_cross_entropy(sigmoid(z), t) wherever fp32 sigmoid has not saturated;
                                                   the clamp at 100 is binary_cross_entropy's clamp of log at -100)
                dz_s = dloss (sigmoid(z_s) - t_s) / S   - the derivative of the UNCLAMPED term, also where the clamp holds
                dh[s,:] = dz_s w,  dw = sum_s dz_s h[s,:],  db = sum_s dz_s

tests/test_cpu_violin.py pins it to what the reference's own code gave (tests/golden/case_violin.npz); the GPU tests compare the
kernels with it."""
import torch

CLAMP = 100.0


def _softmax(s, dim):
    e = torch.exp(s - s.max(dim=dim, keepdim=True).values)
    return e / e.sum(dim=dim, keepdim=True)


def pool_forward(X, m, w):
    """X (S, L, D), m (S, L) 0/1, w (D,) -> dict of float64 tensors."""
    X, m, w = X.double(), m.double(), w.double().reshape(-1)
    att = _softmax((X * w).sum(-1) * m + (1.0 - m) * -1e4, 1)
    return {"att": att, "pooled": (att.unsqueeze(-1) * X).sum(1)}


def pool_backward(X, m, w, dpooled):
    """Upstream dpooled (S, D) -> dX (S, L, D), dw (D,), dw_scale (D,) in float64."""
    X, m, w, dpooled = X.double(), m.double(), w.double().reshape(-1), dpooled.double()
    att = pool_forward(X, m, w)["att"]
    da = (X * dpooled.unsqueeze(1)).sum(-1)
    dot = (att * da).sum(1, keepdim=True)
    ds = att * (da - dot) * m
    # dw sums terms that cancel (ds sums to zero over the frames of a sequence): `dw_scale` is the size of what is summed,
    # att * (|d att| + |<att, d att>|) * |X| - the yardstick for the error of a finite-precision evaluation of dw
    sc = att * (da.abs() + dot.abs()) * m
    return {"dX": att.unsqueeze(-1) * dpooled.unsqueeze(1) + ds.unsqueeze(-1) * w, "ds": ds,
            "dw": (ds.unsqueeze(-1) * X).sum((0, 1)), "dw_scale": (sc.unsqueeze(-1) * X.abs()).sum((0, 1))}


def _softplus(z):
    return z.clamp_min(0.0) + torch.log1p(torch.exp(-z.abs()))


def _sigmoid(z):
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, torch.ones_like(e), e) / (1.0 + e)


def head_forward(h, w, b, t):
    """h (S, K), w (K,), b (1,), t (S,) 0/1 -> logits (S,), terms (S,), loss (), right () in float64."""
    h, w, b = h.double(), w.double().reshape(-1), b.double().reshape(())
    z = (h * w).sum(-1) + b
    one = t.reshape(-1) == 1
    terms = _softplus(torch.where(one, -z, z)).clamp_max(CLAMP)
    return {"logits": z, "terms": terms, "loss": terms.mean(), "right": ((z > 0) == one).sum().double()}


def head_backward(h, w, b, t, dloss=1.0):
    """-> dz (S,), dh (S, K), dw (K,), dw_scale (K,), db () in float64."""
    h, w = h.double(), w.double().reshape(-1)
    z = head_forward(h, w, b, t)["logits"]
    one = t.reshape(-1) == 1
    dz = float(dloss) * torch.where(one, -_sigmoid(-z), _sigmoid(z)) / h.shape[0]      # sigmoid(z) - t, without cancellation
    return {"dz": dz, "dh": dz.unsqueeze(-1) * w, "dw": (dz.unsqueeze(-1) * h).sum(0),
            "dw_scale": (dz.abs().unsqueeze(-1) * h.abs()).sum(0), "db": dz.sum(), "db_scale": dz.abs().sum()}
