"""Float64 restatement of the video-QA head's two attention pools and their gradient, written from the formulas
(HeroForVideoQA.get_modularized_video, model/videoQA.py:36-59) - no autograd, no einsum, no library kernel:

    s_qa[v,a,l] = <X[v,a,l,:], w_qa>,  s_se likewise with w_se;  both through  s * m + (1 - m) * -1e4
    att_qa = softmax over l,  qa_pooled[v,a,:] = sum_l att_qa X          (Nv, A, D)
    att_se = softmax over a,  se_pooled[v,l,:] = sum_a att_se X          (Nv, L, D)

    d att_qa[v,a,l] = <dqa[v,a,:], X[v,a,l,:]>,  d att_se[v,a,l] = <dse[v,l,:], X[v,a,l,:]>
    ds = att * (d att - sum_axis(att * d att)) * m           (softmax backward along its own axis, times d mask_logits / ds)
    dX[v,a,l,:] = att_qa dqa[v,a,:] + att_se dse[v,l,:] + ds_qa w_qa + ds_se w_se
    dw_qa = sum_{v,a,l} ds_qa X,  dw_se = sum_{v,a,l} ds_se X

tests/test_cpu_videoqa.py pins it to what the reference's own code gave (tests/golden/case_videoqa.npz); the GPU tests
compare the kernels with it."""
import torch


def _softmax(s, dim):
    e = torch.exp(s - s.max(dim=dim, keepdim=True).values)
    return e / e.sum(dim=dim, keepdim=True)


def forward(X, m, w_qa, w_se):
    """X (Nv, A, L, D), m (Nv, A, L) 0/1, w_* (D,) -> dict of float64 tensors."""
    X, m, w_qa, w_se = X.double(), m.double(), w_qa.double().reshape(-1), w_se.double().reshape(-1)
    s_qa = (X * w_qa).sum(-1) * m + (1.0 - m) * -1e4
    s_se = (X * w_se).sum(-1) * m + (1.0 - m) * -1e4
    att_qa = _softmax(s_qa, 2)
    att_se = _softmax(s_se, 1)
    return {"att_qa": att_qa, "att_se": att_se,
            "qa_pooled": (att_qa.unsqueeze(-1) * X).sum(2), "se_pooled": (att_se.unsqueeze(-1) * X).sum(1)}


def backward(X, m, w_qa, w_se, dqa, dse):
    """Upstream dqa (Nv, A, D), dse (Nv, L, D) -> dX (Nv, A, L, D), dw_qa (D,), dw_se (D,) in float64."""
    X, m, w_qa, w_se = X.double(), m.double(), w_qa.double().reshape(-1), w_se.double().reshape(-1)
    dqa, dse = dqa.double(), dse.double()
    f = forward(X, m, w_qa, w_se)
    att_qa, att_se = f["att_qa"], f["att_se"]
    da_qa = (X * dqa.unsqueeze(2)).sum(-1)
    da_se = (X * dse.unsqueeze(1)).sum(-1)
    ds_qa = att_qa * (da_qa - (att_qa * da_qa).sum(2, keepdim=True)) * m
    ds_se = att_se * (da_se - (att_se * da_se).sum(1, keepdim=True)) * m
    dX = (att_qa.unsqueeze(-1) * dqa.unsqueeze(2) + att_se.unsqueeze(-1) * dse.unsqueeze(1)
          + ds_qa.unsqueeze(-1) * w_qa + ds_se.unsqueeze(-1) * w_se)
    # dw sums terms that cancel (ds sums to zero along its softmax axis, and the answer copies of a frame are close to each
    # other): `dw_*_scale` is the size of what is summed, att * (|d att| + |<att, d att>|) * |X| - the yardstick for an error
    # of a finite-precision evaluation of dw, which the size of dw itself is not
    sc_qa = att_qa * (da_qa.abs() + (att_qa * da_qa).sum(2, keepdim=True).abs()) * m
    sc_se = att_se * (da_se.abs() + (att_se * da_se).sum(1, keepdim=True).abs()) * m
    return {"dw_qa_scale": (sc_qa.unsqueeze(-1) * X.abs()).sum((0, 1, 2)), "dw_se_scale": (sc_se.unsqueeze(-1) * X.abs()).sum((0, 1, 2)),
            "dX": dX, "dw_qa": (ds_qa.unsqueeze(-1) * X).sum((0, 1, 2)), "dw_se": (ds_se.unsqueeze(-1) * X).sum((0, 1, 2))}
