"""HERO for multiple-choice video question answering, shared by TVQA and How2QA (reference: model/videoQA.py).

Every answer copy of a video runs through the cross-modal encoder with `[sep] question [sep] answer` appended to each
subtitle; its frame rows and the QA token embeddings then go through the temporal transformer as ONE sequence
`[frames ; qa tokens]`.  Two attention pools read the frame rows of that output - one over the frames of each copy (the
answer logits), one over the copies of each frame (the start / end logits): hero_amd.qa.QaPoolFn, one HIP kernel each way."""
import copy
from collections import defaultdict

import torch
from torch import nn
from torch.nn import functional as F

from .. import _lib as L
from .. import functional as HF
from .. import qa as QA
from .layers import MLPLayer
from .model import HeroModel
from .modeling_utils import mask_logits

_TASKS = ("tvqa", "how2qa")


def _mlp_narrow(mlp, x):
    """MLPLayer with a 1- or 2-wide output.  Linear -> GELU -> LayerNorm run on the kernels as in MLPLayer.forward; hero_gemm
    takes output widths that are multiples of 4, so the final [rows, 2D] x [2D, 1 | 2] projection is a torch matvec in fp32 (a
    few thousand multiply-adds per row, capturable like the cross-entropies behind it)."""
    x = HF.cast(x, HF.compute_dtype())
    h = HF.linear(x, mlp.linear_1.weight, mlp.linear_1.bias, act=L.ACT_GELU)
    h = HF.cast(mlp.LayerNorm(h), torch.float32)
    return F.linear(h, mlp.linear_2.weight, mlp.linear_2.bias)


class HeroForVideoQA(HeroModel):
    def __init__(self, config, vfeat_dim, max_frm_seq_len):
        super().__init__(config, vfeat_dim, max_frm_seq_len)
        hsz = config.c_config.hidden_size
        self.qa_pool = nn.Linear(in_features=hsz, out_features=1, bias=False)
        self.qa_pred_head = MLPLayer(hsz, 1)
        # tvqa / how2qa also annotate the start and end frame of the answer's evidence
        self.st_ed_pool = copy.deepcopy(self.qa_pool)
        self.st_ed_pred_head = MLPLayer(hsz, 2)

    fused_pool = True       # both attention pools as one HIP kernel (hero_qa_pool_*); False / outside its envelope: PyTorch ops

    def get_modularized_video(self, frame_embeddings, frame_mask):
        """The PyTorch formulation (model/videoQA.py:36-59): the comparison side of the parity tests and the route of shapes
        outside the kernels' envelope.  frame_embeddings (Nv, A, L, D) fp32, frame_mask (Nv, A, L) fp32 ->
        (st_ed_pooled (Nv, L, D), qa_pooled (Nv, A, D))."""
        st_ed_scores = self.st_ed_pool(frame_embeddings)                          # (Nv, A, L, 1)
        qa_scores = self.qa_pool(frame_embeddings)
        st_ed_att = F.softmax(mask_logits(st_ed_scores, frame_mask.unsqueeze(-1)), dim=1)
        qa_att = F.softmax(mask_logits(qa_scores, frame_mask.unsqueeze(-1)), dim=2)
        st_ed_pooled = torch.einsum("vqlm,vqld->vlmd", st_ed_att, frame_embeddings)
        qa_pooled = torch.einsum("vqlm,vqld->vqmd", qa_att, frame_embeddings)
        return st_ed_pooled.squeeze(2), qa_pooled.squeeze(2)

    def forward(self, batch, task="tvqa", compute_loss=True):
        batch = defaultdict(lambda: None, batch)
        if task not in _TASKS:
            raise ValueError(f"Unrecognized task: {task}")
        enc = self.v_encoder
        targets = batch["targets"].squeeze(-1)
        c_attn_masks, qa_attn_masks = batch["c_attn_masks"], batch["qa_attn_masks"]
        num_videos = len(targets)
        S, num_frames = c_attn_masks.shape
        n_qa = qa_attn_masks.shape[1]
        if S % num_videos:
            raise ValueError("video QA batch: %d answer copies do not divide over %d videos" % (S, num_videos))
        A = S // num_videos
        limit = L.lib().hero_attention_max_len(L.BF16 if HF.compute_dtype() == torch.bfloat16 else L.F32,
                                               int(torch.is_grad_enabled()))
        if num_frames + n_qa > limit:
            raise ValueError("video QA: %d frames + %d QA tokens = %d positions, the attention kernels take at most %d in %s"
                             % (num_frames, n_qa, num_frames + n_qa, limit, HF.compute_dtype()))
        # (num_videos * A, num_frames, hidden)
        frame_embeddings = enc.forward_repr(batch, encode_clip=False)
        frame_embeddings = enc.c_encoder.embeddings(frame_embeddings, position_ids=None)
        qa_embeddings = enc.f_encoder._compute_txt_embeddings(batch["qa_input_ids"], batch["qa_pos_ids"], txt_type_ids=None)
        frame_qa_embeddings = torch.cat((frame_embeddings, qa_embeddings), dim=1)
        frame_qa_attn_mask = HF.memo("qa_cat_mask", (c_attn_masks, qa_attn_masks),
                                     lambda: torch.cat((c_attn_masks, qa_attn_masks), dim=1))
        fused_video_qa = enc.c_encoder.forward_encoder(frame_qa_embeddings, frame_qa_attn_mask)
        hid = fused_video_qa.shape[-1]
        video_masks = HF.memo("mask_f32", (c_attn_masks,), lambda: c_attn_masks.to(torch.float32), spec=(L.DERIVE_F32, 0, 0, 0))
        if self.fused_pool and QA.in_envelope(A, num_frames, num_frames + n_qa, hid):
            qa_pooled, st_ed_pooled = QA.QaPoolFn.apply(fused_video_qa, video_masks, self.qa_pool.weight, self.st_ed_pool.weight,
                                                        A, num_frames)
        else:
            video_embeddings = HF.cast(fused_video_qa, torch.float32)[:, :num_frames, :]
            st_ed_pooled, qa_pooled = self.get_modularized_video(video_embeddings.view(num_videos, A, num_frames, hid),
                                                                 video_masks.view(num_videos, A, num_frames))
        first = video_masks.view(num_videos, A, num_frames)[:, 0]
        pred_st_ed = _mlp_narrow(self.st_ed_pred_head, st_ed_pooled)
        st_prob = mask_logits(pred_st_ed[:, :, 0], first)
        ed_prob = mask_logits(pred_st_ed[:, :, 1], first)
        logits = _mlp_narrow(self.qa_pred_head, qa_pooled).squeeze(-1)
        if not compute_loss:
            return logits
        ts_targets = batch["ts_targets"]
        st_loss = F.cross_entropy(st_prob, ts_targets[:, 0], reduction="mean", ignore_index=-1)
        ed_loss = F.cross_entropy(ed_prob, ts_targets[:, 1], reduction="mean", ignore_index=-1)
        temporal_loss = (st_loss + ed_loss) / 2.
        qa_loss = F.cross_entropy(logits, targets, reduction="mean", ignore_index=-1)
        return qa_loss, temporal_loss
