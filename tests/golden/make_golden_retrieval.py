#!/usr/bin/env python3
"""Golden vectors of the full-corpus retrieval (eval_vcmr.py:143-338) by importing the *reference* HERO code with the tiny
weights of tests/golden/tiny_model.npz.

Container-only (needs the reference checkout), exactly like make_golden.py, whose stubs and synthetic collate it reuses.
Writes tests/golden/case_retrieval.npz:

  b<i>.in.*       three video batches of different clip lengths (synthetic collate)
  in.query_*      the query batch, in.gt_vidx the ground-truth video of each query
  corpus, corpus_masks   the padded corpus tensor / masks of eval_vcmr.py:185-203 (trimmed to the longest clip)
  mod_q           model.encode_txt_inputs(..., attn_layer=q_feat_attn)
  q2video_scores, st_logits, ed_logits     get_pred_from_raw_query(cross=True, val_gather_gpus=False)      (:232-235)
  band.<L>.<min_l>.<max_l>                 generate_min_max_length_mask                                    (:292-294)
  vr_scores, vr_indices                    exp(q2c_alpha * s), torch.topk                                  (:266-269)
  vcmr_scores, vcmr_flat                   einsum, band mask, sort, first max_before_nms                   (:290-312)
  svmr_triples                             find_max_triples_from_upper_triangle_product                    (:327-338)
  cfg                                      [q2c_alpha, max_vcmr_video, min_pred_l, max_pred_l, max_before_nms, max_clip_len]

The inputs are accepted only if no two scores inside (or at the edge of) a kept range are equal: asserted below.

Run:  python tests/golden/make_golden_retrieval.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G            # noqa: E402  (stubs + synthetic collate)

ALPHA, K, MIN_L, MAX_L, TOP_N = 20, 3, 1, 4, 12
BANDS = [(12, 1, 4), (12, 2, 16), (5, 0, 3), (1, 2, 16), (100, 2, 16)]


def strictly_decreasing(x, what):
    x = np.asarray(x, dtype=np.float64)
    assert (np.diff(x, axis=1) < 0).all(), "tie inside the kept range of " + what


def main():
    G.install_stubs()
    sys.path.insert(0, G.REF)
    from model.vcmr import HeroForVcmr            # noqa: reference import
    from utils.tvr_eval_utils import (find_max_triples_from_upper_triangle_product,   # noqa: reference import
                                      generate_min_max_length_mask)

    z = np.load(os.path.join(HERE, "tiny_model.npz"), allow_pickle=False)
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    model = HeroForVcmr.from_pretrained(
        os.path.join(HERE, "tiny_config.json"), state_dict=sd, vfeat_dim=G.VFEAT, max_frm_seq_len=G.MAX_FRM,
        lw_neg_ctx=8.0, lw_neg_q=8.0, lw_st_ed=0.01, ranking_loss_type="hinge", use_hard_negative=False,
        hard_pool_size=20, margin=0.1, use_all_neg=True, drop_svmr_prob=0.0)
    model.eval()
    gen = torch.Generator().manual_seed(23)
    d = {}
    batches = [
        G.synth_video_batch(gen, subs=[[([0, 1, 2], 6), ([3, 4], 5), ([6, 7, 8], 7)], [([0, 1], 4), ([2, 3, 4, 5], 7)]], n_frames=[9, 6]),
        G.synth_video_batch(gen, subs=[[([0, 1, 2, 3], 5), ([5, 6], 3), ([8, 9, 10, 11], 6)], [([1, 2, 3], 5)],
                                       [([0], 2), ([1, 2], 8), ([5, 6, 7, 8, 9], 6)]], n_frames=[12, 5, 10]),
        G.synth_video_batch(gen, subs=[[([0, 1, 2], 4)], [([0, 1, 2], 6), ([3, 4, 5, 6], 5)]], n_frames=[4, 7]),
    ]
    n_videos = sum(b["c_attn_masks"].shape[0] for b in batches)
    max_clip_len = G.MAX_FRM
    total = total_masks = None
    seen, at = 0, 0
    with torch.no_grad():
        for i, b in enumerate(batches):
            for k_, v in G.pack_batch(b).items():
                d["b%d.%s" % (i, k_)] = v
            emb = model.v_encoder(b, "repr")
            cm = b["c_attn_masks"]
            cl = emb.size(-2)
            assert cl <= max_clip_len
            if total is None:                                       # eval_vcmr.py:185-194
                total = torch.zeros((n_videos, max_clip_len, emb.size(-1)), dtype=emb.dtype)
                total_masks = torch.zeros((n_videos, max_clip_len), dtype=cm.dtype)
            idx = torch.arange(at, at + emb.size(0))
            total[idx, :cl] = emb                                   # :195-199
            total_masks[idx, :cl] = cm
            seen = max(seen, cl)
            at += emb.size(0)
        total, total_masks = total[:, :seen, :], total_masks[:, :seen]        # :202-203
        qi, qp, qm = G.synth_queries(gen, 5, [5, 7, 4, 6, 3])
        gt = torch.tensor([1, 4, 0, 6, 2])
        d["in.query_input_ids"], d["in.query_pos_ids"], d["in.query_attn_masks"], d["in.gt_vidx"] = qi.numpy(), qp.numpy(), qm.numpy(), gt.numpy()
        d["corpus"], d["corpus_masks"] = total.numpy(), total_masks.numpy()
        d["mod_q"] = model.encode_txt_inputs(qi, qp, qm, attn_layer=model.q_feat_attn).numpy()
        q2v, st, ed = model.get_pred_from_raw_query(total, total_masks, query_input_ids=qi, query_pos_ids=qp, query_attn_masks=qm,
                                                    cross=True, val_gather_gpus=False)                     # :232-235
        d["q2video_scores"], d["st_logits"], d["ed_logits"] = q2v.numpy(), st.numpy(), ed.numpy()
        st_p, ed_p = F.softmax(st, dim=-1), F.softmax(ed, dim=-1)                                          # :237-238
        for (ln, a, b_) in BANDS:
            d["band.%d.%d.%d" % (ln, a, b_)] = generate_min_max_length_mask((2, 3, ln, ln), min_l=a, max_l=b_)[0, 0]
        e = torch.exp(ALPHA * q2v.float())                                                                 # :263-269
        strictly_decreasing(torch.sort(e, dim=1, descending=True)[0][:, :K + 1], "the video scores")
        vs, vi = torch.topk(e, K, dim=1, largest=True)
        d["vr_scores"], d["vr_indices"] = vs.numpy(), vi.numpy()
        rows = torch.arange(len(st_p)).unsqueeze(1)
        sk, ek = st_p[rows, vi], ed_p[rows, vi]                                                            # :284-288
        prod = torch.einsum("qvm,qv,qvn->qvmn", sk, vs, ek)                                                # :290-291
        prod *= torch.from_numpy(generate_min_max_length_mask(prod.shape, min_l=MIN_L, max_l=MAX_L))      # :292-297
        ss, si = torch.sort(prod.reshape(len(prod), -1), dim=1, descending=True)                           # :300-304
        strictly_decreasing(ss[:, :TOP_N + 1], "the VCMR moments")
        assert float(ss[:, TOP_N].min()) > 0
        d["vcmr_scores"], d["vcmr_flat"] = ss[:, :TOP_N].numpy(), si[:, :TOP_N].numpy()                   # :306-312
        r1 = torch.arange(len(st_p))
        sp = np.einsum("bm,bn->bmn", st_p[r1, gt].numpy(), ed_p[r1, gt].numpy())                           # :241-258, 327-329
        sp *= generate_min_max_length_mask(sp.shape, min_l=MIN_L, max_l=MAX_L)                             # :330-334
        n_sv = 8                                   # the shortest ground-truth video has 5 frames: 9 in-band moments with a positive score
        tri = np.stack(find_max_triples_from_upper_triangle_product(sp, top_n=n_sv + 1, prob_thd=None))   # :335-338
        strictly_decreasing(tri[:, :, 2], "the SVMR moments")
        assert tri[:, :, 2].min() > 0
        d["svmr_triples"] = tri[:, :n_sv]
        d["cfg"] = np.array([ALPHA, K, MIN_L, MAX_L, TOP_N, max_clip_len, n_sv])
    np.savez_compressed(os.path.join(HERE, "case_retrieval.npz"), **d)
    print("case_retrieval.npz  corpus", tuple(total.shape), " vr", d["vr_indices"].tolist(), " vcmr top", d["vcmr_scores"][:, 0].tolist())
    print("bytes", os.path.getsize(os.path.join(HERE, "case_retrieval.npz")))


if __name__ == "__main__":
    main()
