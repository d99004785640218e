"""HERO for video-and-language inference, VIOLIN (reference: model/violin.py).

Every (video, statement) copy runs through the cross-modal encoder with `[sep] statement` appended to each subtitle; its
frame rows and the statement's token embeddings then go through the temporal transformer as ONE sequence
`[frames ; statement tokens]`.  One attention pool reads the frame rows of that output (hero_amd.violin.FramePoolFn), an
MLPLayer(hsz, 1) turns the pooled vector into a logit, and the loss is binary cross-entropy on its sigmoid - the projection,
the loss and its gradient are one HIP kernel each way (hero_amd.violin.BceHeadFn)."""
from collections import defaultdict

import torch
from torch import nn
from torch.nn import functional as F

from .. import _lib as L
from .. import functional as HF
from .. import violin as V
from .layers import MLPLayer
from .model import HeroModel
from .modeling_utils import mask_logits
from .videoQA import _mlp_narrow


class HeroForViolin(HeroModel):
    def __init__(self, config, vfeat_dim, max_frm_seq_len):
        super().__init__(config, vfeat_dim, max_frm_seq_len)
        hsz = config.c_config.hidden_size
        self.violin_pool = nn.Linear(in_features=hsz, out_features=1, bias=False)
        self.violin_pred_head = MLPLayer(hsz, 1)

    fused_head = True       # pool and classifier tail on the HIP kernels (hero_frame_pool_*, hero_bce_head_*); False / outside
                            # their envelopes / CPU tensors: PyTorch ops

    def get_modularized_video(self, frame_embeddings, frame_mask):
        """The PyTorch formulation (model/violin.py:30-47): the comparison side of the parity tests and the route of shapes
        outside the kernels' envelope.  frame_embeddings (Nv, L, D), frame_mask (Nv, L) -> (Nv, D)."""
        violin_attn_scores = self.violin_pool(frame_embeddings)                   # (Nv, L, 1)
        violin_attn_scores = F.softmax(mask_logits(violin_attn_scores, frame_mask.unsqueeze(-1)), dim=1)
        violin_pooled_video = torch.einsum("vlm,vld->vmd", violin_attn_scores, frame_embeddings)
        return violin_pooled_video.squeeze(1)

    def forward(self, batch, task="violin", compute_loss=True):
        batch = defaultdict(lambda: None, batch)
        if task != "violin":
            raise ValueError(f"Unrecognized task: {task}")
        enc = self.v_encoder
        c_attn_masks, q_attn_masks = batch["c_attn_masks"], batch["q_attn_masks"]
        S, num_frames = c_attn_masks.shape
        n_q = q_attn_masks.shape[1]
        limit = L.lib().hero_attention_max_len(L.BF16 if HF.compute_dtype() == torch.bfloat16 else L.F32,
                                               int(torch.is_grad_enabled()))
        if num_frames + n_q > limit:
            raise ValueError("violin: %d frames + %d statement tokens = %d positions, the attention kernels take at most %d in %s"
                             % (num_frames, n_q, num_frames + n_q, limit, HF.compute_dtype()))
        # (num_videos * statements, num_frames, hidden)
        frame_embeddings = enc.forward_repr(batch, encode_clip=False)
        frame_embeddings = enc.c_encoder.embeddings(frame_embeddings, position_ids=None)
        q_embeddings = enc.f_encoder._compute_txt_embeddings(batch["q_input_ids"], batch["q_pos_ids"], txt_type_ids=None)
        frame_q_embeddings = torch.cat((frame_embeddings, q_embeddings), dim=1)
        frame_q_attn_mask = HF.memo("violin_cat_mask", (c_attn_masks, q_attn_masks),
                                    lambda: torch.cat((c_attn_masks, q_attn_masks), dim=1))
        fused_video_q = enc.c_encoder.forward_encoder(frame_q_embeddings, frame_q_attn_mask)
        hid = fused_video_q.shape[-1]
        video_masks = HF.memo("mask_f32", (c_attn_masks,), lambda: c_attn_masks.to(torch.float32), spec=(L.DERIVE_F32, 0, 0, 0))
        targets = batch["targets"]
        head = self.violin_pred_head
        if (self.fused_head and fused_video_q.is_cuda and V.pool_in_envelope(num_frames, num_frames + n_q, hid)
                and V.head_in_envelope(S, head.linear_2.in_features)):
            pooled = V.FramePoolFn.apply(fused_video_q, video_masks, self.violin_pool.weight, num_frames)
            h = HF.linear(HF.cast(pooled, HF.compute_dtype()), head.linear_1.weight, head.linear_1.bias, act=L.ACT_GELU)
            h = head.LayerNorm(h)
            t = targets.reshape(-1) if targets is not None else torch.zeros(S, dtype=torch.long, device=h.device)
            violin_loss, logits = V.BceHeadFn.apply(h, head.linear_2.weight, head.linear_2.bias, t)
            return violin_loss if compute_loss else logits.unsqueeze(-1)
        video_embeddings = HF.cast(fused_video_q, torch.float32)[:, :num_frames, :]
        logits = _mlp_narrow(head, self.get_modularized_video(video_embeddings, video_masks))
        if not compute_loss:
            return logits
        scores = torch.sigmoid(logits).squeeze(-1)
        return F.binary_cross_entropy(scores, targets.squeeze(-1).to(dtype=scores.dtype), reduction="mean")
