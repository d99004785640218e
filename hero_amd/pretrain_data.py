"""Pre-training batches drawn ON THE DEVICE: one clean video batch -> the MLM, MFM and FOM batch (device half of the
pre-training collates of hero_amd/collate.py).

The reference draws the masks in the DataLoader workers, one random.random() per subtitle token (data/mlm.py:21-58) and per
frame (data/mfm.py:19-25, data/fom.py:96-115), with one dataset and loader per task over the same videos.  `PretrainMasker`
takes ONE clean batch that is already on the device - video_collate's tensors plus DeviceCollate's length slots - and makes
the three task batches with kernels (hero_amd/csrc/pretrain_mask.hip): a fresh draw per step, no host work.  The draw is
counter-based and keyed by a device seed word, so a captured `draw()` serves every seed; its exact statement is in that file's
header and, in integer arithmetic, in tests/pretrain_mask_reference.py.

Outputs live at fixed addresses with fixed capacities (`static_entries()`):
    input_ids [T, max_sl] int64, txt_mask_tgt [T, Lf] bool, txt_labels [T * (max_sl - 1)] int64 (-1 behind the count),
    txt_mask_rows [T * (max_sl - 1)] int32 flat indices into [T * Lf] (-1 behind the count)
    c_v_masks [B, NF] bool, f_v_masks [T, max_vl] bool, feat_targets [B * NF, D] fp32 (zero rows behind the count),
    c_v_feats [B, NF, D] / f_v_feats [T, max_vl, D] fp32 masked COPIES (the clean batch stays clean for the next task)
    shuffled_orders, targets [B, NF] int64
    counts [2] int32 = (masked tokens, masked frames)
`mlm_batch()` / `mfm_batch()` / `fom_batch()` return dicts with the reference collates' keys; the compact tensors are narrowed
to their counts there, which costs one host read of the counts per draw (the model synchronises on `nonzero` of the masks
for these batches anyway).

The FIXED-CAPACITY forms (`draw_fixed`, `static_batch`) read nothing on the host: the loss heads take the
device counts (hero_ce_counted_*, hero_nce_pack_*), the compact tensors keep a capacity of `row_capacity(...)` rows, and a
captured step replays on a fresh draw per micro-step (hero_amd.step.TrainStep draws for a batch that carries `_masker`).
"""
import math

import torch

from . import _lib as L
from . import functional as HF
from .collate import DeviceCollate

SITES = {"mlm": 0x4D4C4D, "mfm": 0x4D464D, "fom": 0x464F4D}       # the per-task site words ("MLM", "MFM", "FOM")
SEED_STEP = 0x9E3779B97F4A7C15                                     # advance(): seed += this (mod 2^64)
_LENGTH_KEYS = ("sub_nfrm", "sub_ntok", "sub_frm_off", "sub_frm", "vid_sub_off", "vid_nfrm")


def threshold(p):
    """floor(p * 2^32) in exact arithmetic (a scaling by a power of two): p = 1 gives 2^32, which selects everything."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("probability %r outside [0, 1]" % (p,))
    return int(math.floor(p * 4294967296.0))


def _signed(word):
    word &= (1 << 64) - 1
    return word - (1 << 64) if word >= 1 << 63 else word


class PretrainMasker:
    def __init__(self, T, max_sl, max_vl, out_size, B, NF, vfeat_dim, device, mask_id, v_range, cls_id, mlm_prob=0.15, mfm_prob=0.15,
                 fom_prob=0.15, sites=None, seed=0, mlm_rows=None, mfm_rows=None):
        self.T, self.max_sl, self.max_vl, self.Lf, self.B, self.NF, self.D = T, max_sl, max_vl, out_size, B, NF, vfeat_dim
        self.device = torch.device(device)
        self.mask_id, self.v_range, self.cls_id = int(mask_id), (int(v_range[0]), int(v_range[1])), int(cls_id)
        self.thr = {"mlm": threshold(mlm_prob), "mfm": threshold(mfm_prob), "fom": threshold(fom_prob)}
        self.sites = dict(SITES, **(sites or {}))
        self.cap = T * (max_sl - 1)
        z = lambda *shape, dt: torch.zeros(*shape, dtype=dt, device=self.device)      # noqa: E731
        self.seed = z(1, dt=torch.int64)
        self.counts = z(2, dt=torch.int32)
        self.input_ids = z(T, max_sl, dt=torch.int64)
        self.txt_mask_tgt = z(T, out_size, dt=torch.bool)
        self.txt_labels = z(max(self.cap, 1), dt=torch.int64)
        self.txt_mask_rows = z(max(self.cap, 1), dt=torch.int32)
        self.c_v_masks = z(B, NF, dt=torch.bool)
        self.f_v_masks = z(T, max_vl, dt=torch.bool)
        self.feat_targets = z(B * NF, vfeat_dim, dt=torch.float32)
        self.c_v_feats = z(B, NF, vfeat_dim, dt=torch.float32)
        self.f_v_feats = z(T, max_vl, vfeat_dim, dt=torch.float32)
        self.shuffled_orders = z(B, NF, dt=torch.int64)
        self.targets = z(B, NF, dt=torch.int64)
        self._row_src = z(2 * B * NF + T * max_vl, dt=torch.int32)
        # fixed-capacity forms: row capacities of the loss heads, the MFM partition, what the heads read besides the draws
        self.mlm_rows = self._capacity("mlm_rows", mlm_rows, self.cap, mlm_prob, T)
        self.mfm_rows = self._capacity("mfm_rows", mfm_rows, B * NF, mfm_prob, B)
        self.mfm_order = z(B * NF, dt=torch.int32)
        self.mfm_rank = z(B * NF, dt=torch.int32)
        self.nce_labels = torch.arange(max(self.mfm_rows, 1), dtype=torch.int64, device=self.device)
        self.overflow = z(2, dt=torch.int64)          # draws whose (masked tokens, masked frames) exceeded the capacity
        self._clean, self._host_counts, self._lengths_src, self._static = None, None, None, {}
        self.set_seed(seed)

    @classmethod
    def for_batch(cls, batch, device, mask_id, v_range, cls_id, **kw):
        """Buffers sized for a (host or device) batch of video_collate."""
        T, max_vl, D = batch["f_v_feats"].shape
        B, NF = batch["c_attn_masks"].shape
        return cls(T, batch["f_sub_input_ids"].shape[1], max_vl, batch["f_attn_masks"].shape[1], B, NF, D, device, mask_id, v_range,
                   cls_id, **kw)

    @staticmethod
    def row_capacity(n, p, forced):
        """Rows kept for a mask over at most n selectable positions drawn with probability p, plus `forced` selections of the
        at-least-one rule: mean + six standard deviations of the binomial (a tail bound: about 1e-9 per draw by the normal
        approximation - not a measurement), rounded up to the GEMM's 8-row granularity, never more than n."""
        if not 0.0 <= p <= 1.0 or n < 0 or forced < 0:
            raise ValueError("row_capacity: n, forced >= 0 and p in [0, 1]")
        rows = int(math.ceil(n * p + 6.0 * math.sqrt(n * p * (1.0 - p)))) + int(forced)
        return min(int(n), (rows + 7) // 8 * 8)

    def _capacity(self, name, given, n, p, forced):
        rows = self.row_capacity(n, p, forced) if given is None else int(given)
        if not (1 <= rows <= n or n == 0):
            raise ValueError("PretrainMasker: %s = %d outside [1, %d]" % (name, rows, n))
        return rows

    # ---- the seed word (device ops: stream-ordered with the draws) -----------------------------------------------------
    def set_seed(self, s):
        self.seed.fill_(_signed(int(s)))
        return self

    def advance(self):
        self.seed.add_(_signed(SEED_STEP))             # two's complement: the sum mod 2^64
        return self

    # ---- the draw ------------------------------------------------------------------------------------------------------
    def _lengths(self, src):
        slots = src._in if isinstance(src, DeviceCollate) else src
        out = {}
        for k in _LENGTH_KEYS:
            t = slots[k]
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32):
                raise TypeError("PretrainMasker.draw: %s must be an int32 device tensor (DeviceCollate's slots, or copies of "
                                "batch['lengths'] made by the caller): draw() only launches" % k)
            out[k] = t
        if out["sub_nfrm"].numel() != self.T or out["sub_ntok"].numel() != self.T or out["sub_frm_off"].numel() < self.T + 1 \
                or out["vid_nfrm"].numel() != self.B or out["vid_sub_off"].numel() < self.B + 1:
            raise ValueError("PretrainMasker.draw: length arrays of another batch shape")
        return out

    def draw(self, clean_batch, collate_or_lengths, tasks=("mlm", "mfm", "fom")):
        """Launch the draws of `tasks` for the clean device batch: kernels only - no host data, no synchronisation, nothing
        allocated (capturable in a hipGraph).  The clean tensors are only read."""
        self._rewritten(self._launch(clean_batch, collate_or_lengths, tasks) + [self.counts])
        self._clean, self._lengths_src = clean_batch, collate_or_lengths
        return self

    def _launch(self, clean_batch, collate_or_lengths, tasks):
        """The kernels of `tasks`; returns the tensors they wrote."""
        ln, s, lib = self._lengths(collate_or_lengths), L.stream(), L.lib()
        written = []
        for task in tasks:
            if task == "mlm":
                ids = clean_batch["f_sub_input_ids"]
                if tuple(ids.shape) != (self.T, self.max_sl) or ids.dtype != torch.int64:
                    raise ValueError("PretrainMasker.draw: f_sub_input_ids must be int64 [%d, %d]" % (self.T, self.max_sl))
                L.check(lib.hero_mlm_mask(L.ptr(ids), L.ptr(ln["sub_nfrm"]), L.ptr(ln["sub_ntok"]), L.ptr(self.seed), self.sites["mlm"],
                                          self.thr["mlm"], self.mask_id, self.v_range[0], self.v_range[1], self.cls_id,
                                          L.ptr(self.input_ids), L.ptr(self.txt_mask_tgt), L.ptr(self.txt_labels),
                                          L.ptr(self.txt_mask_rows), L.ptr(self.counts[0:1]), self.T, self.max_sl, self.Lf, s))
                written += [self.input_ids, self.txt_mask_tgt, self.txt_labels, self.txt_mask_rows]
            elif task == "mfm":
                c = clean_batch["c_v_feats"]
                if tuple(c.shape) != (self.B, self.NF, self.D) or c.dtype != torch.float32:
                    raise ValueError("PretrainMasker.draw: c_v_feats must be fp32 [%d, %d, %d]" % (self.B, self.NF, self.D))
                L.check(lib.hero_mfm_mask(L.ptr(c), L.ptr(ln["vid_nfrm"]), L.ptr(ln["vid_sub_off"]), L.ptr(ln["sub_frm_off"]),
                                          L.ptr(ln["sub_frm"]), L.ptr(self.seed), self.sites["mfm"], self.thr["mfm"],
                                          L.ptr(self.c_v_masks), L.ptr(self.f_v_masks), L.ptr(self.feat_targets),
                                          L.ptr(self.counts[1:2]), L.ptr(self.c_v_feats), L.ptr(self.f_v_feats), L.ptr(self._row_src),
                                          self.T, self.max_vl, self.B, self.NF, self.D, s))
                written += [self.c_v_masks, self.f_v_masks, self.feat_targets, self.c_v_feats, self.f_v_feats]
            elif task == "fom":
                L.check(lib.hero_fom_shuffle(L.ptr(ln["vid_nfrm"]), L.ptr(self.seed), self.sites["fom"], self.thr["fom"],
                                             L.ptr(self.shuffled_orders), L.ptr(self.targets), self.B, self.NF, s))
                written += [self.shuffled_orders, self.targets]
            else:
                raise ValueError("PretrainMasker.draw: unknown task %r (mlm, mfm, fom)" % (task,))
        return written

    # ---- the fixed-capacity forms ----------------------------------------------------------------------------------------
    def draw_fixed(self, clean_batch, collate_or_lengths, task):
        """draw() of ONE task for a consumer that holds everything by address (a captured step): the same kernels, plus the
        stable partition of the frame mask for MFM and the overflow counter.  Memo entries are kept - captured graphs hold the
        derived tensors (`row_index` / `seg_order` of input_ids, `c_v_mask_rows`) - and redone in place from the new draw;
        only row lists taken with torch.nonzero for the compact forms go (their shape follows the mask, no graph can hold
        them).  Launches and stream-ordered device ops only: no host read.  Not inside a capture (it moves version counters
        and re-keys memo entries, which a replay would not do)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("PretrainMasker.draw_fixed: call it in front of the capture / replay, not inside")
        written = self._launch(clean_batch, collate_or_lengths, (task,))
        if task == "mlm":
            self.overflow[0:1] += self.counts[0:1] > self.mlm_rows
        elif task == "mfm":
            HF.mask_partition(self.c_v_masks, self.mfm_order, self.mfm_rank, self.counts[1:2])     # the count again: same value
            self.overflow[1:2] += self.counts[1:2] > self.mfm_rows
            written += [self.mfm_order, self.mfm_rank]
        written.append(self.counts)
        torch._C._increment_version(written)
        HF.forget_memo(written, tags=("mask_rows",))
        HF.restamp_memo(HF.refresh_memo(sources=written))
        self._host_counts = None
        self._clean, self._lengths_src = clean_batch, collate_or_lengths
        return self

    def redraw(self, task):
        """advance() + draw_fixed() on the clean batch and lengths of the last draw: a fresh mask for the next micro-step."""
        self._need_clean()
        return self.advance().draw_fixed(self._clean, self._lengths_src, task)

    def static_batch(self, task):
        """The batch of `task` ('mlm', 'mfm', 'fom') in its fixed-capacity form: ONE dict object per task (a captured step
        accepts only the object it was captured on), the clean batch's keys plus the draw's tensors at fixed addresses and
        the device counts.  `_static_buffers` keeps host-derived pack plans away from it, `_masker` lets TrainStep draw."""
        if task not in self._static:
            out = dict(self._need_clean())
            if task == "mlm":
                c = self._clean
                out.update(input_ids=self.input_ids, position_ids=c["f_sub_pos_ids"], v_feat=c["f_v_feats"], attn_masks=c["f_attn_masks"],
                           gather_index=c["f_gather_index"], txt_mask_tgt=self.txt_mask_tgt, txt_mask_rows=self.txt_mask_rows[:self.mlm_rows],
                           txt_labels=self.txt_labels[:self.mlm_rows])
            elif task == "mfm":
                out.update(f_v_feats=self.f_v_feats, c_v_feats=self.c_v_feats, f_v_masks=self.f_v_masks, c_v_masks=self.c_v_masks,
                           feat_targets=self.feat_targets, mfm_order=self.mfm_order, mfm_rank=self.mfm_rank, nce_labels=self.nce_labels)
            elif task == "fom":
                out.update(shuffled_orders=self.shuffled_orders, targets=self.targets)
            else:
                raise ValueError("PretrainMasker.static_batch: unknown task %r (mlm, mfm, fom)" % (task,))
            out.update(mask_counts=self.counts, _static_buffers=True, _masker=self)
            self._static[task] = out
        return self._static[task]

    def _rewritten(self, tensors):
        # raw kernels wrote them: caches keyed on (address, version) must miss (DeviceCollate.rebuild does the same), and what
        # was derived from the previous masks goes - a new mask has another number of rows, refresh_memo() could not redo it
        torch._C._increment_version(tensors)
        if not torch.cuda.is_current_stream_capturing():
            HF.forget_memo(tensors)
        self._host_counts = None

    def note_replay(self, clean_batch=None):
        """After a captured draw() was replayed: the outputs changed behind torch's back - move their versions and forget
        the counts read for the previous draw."""
        self._rewritten(list(self.static_entries().values()))
        if clean_batch is not None:
            self._clean = clean_batch
        return self

    # ---- the batches -----------------------------------------------------------------------------------------------------
    def _counts(self):
        if self._host_counts is None:
            self._host_counts = [int(c) for c in self.counts.tolist()]          # the one host read
        return self._host_counts

    def _need_clean(self):
        if self._clean is None:
            raise RuntimeError("PretrainMasker: no draw() yet")
        return self._clean

    def mlm_batch(self):
        """The keys of the reference's mlm_collate (data/mlm.py:169-175)."""
        c = self._need_clean()
        return {"input_ids": self.input_ids, "position_ids": c["f_sub_pos_ids"], "v_feat": c["f_v_feats"], "attn_masks": c["f_attn_masks"],
                "gather_index": c["f_gather_index"], "txt_mask_tgt": self.txt_mask_tgt, "txt_labels": self.txt_labels[:self._counts()[0]]}

    def mfm_batch(self):
        """The clean batch's keys with the masked feature copies, plus f_v_masks, c_v_masks, feat_targets (data/mfm.py:77-97)."""
        out = dict(self._need_clean())
        out.update(f_v_feats=self.f_v_feats, c_v_feats=self.c_v_feats, f_v_masks=self.f_v_masks, c_v_masks=self.c_v_masks,
                   feat_targets=self.feat_targets[:self._counts()[1]])
        return out

    def fom_batch(self, pairs=True):
        """The clean batch's keys plus shuffled_orders, targets and - pairs=True, as the reference's collate returns them although
        no model reads them - reordered_frame_idx / binary_targets (data/fom.py:64-92), derived with torch ops (they synchronise)."""
        out = dict(self._need_clean())
        out.update(shuffled_orders=self.shuffled_orders, targets=self.targets)
        if pairs:
            t = self.targets
            sel = t != -1
            upper = torch.ones(self.NF, self.NF, dtype=torch.bool, device=t.device).triu_(1)
            b, i, j = torch.nonzero(sel.unsqueeze(2) & sel.unsqueeze(1) & upper, as_tuple=True)     # (clip, i, j) row-major: the reference's loops
            pi, pj = b * self.NF + i, b * self.NF + j
            ti, tj = t[b, i], t[b, j]
            out["reordered_frame_idx"] = torch.stack([pi, pj, pj, pi], 1).reshape(-1)
            out["binary_targets"] = torch.stack([ti <= tj, tj <= ti], 1).reshape(-1).long()
        return out

    def static_entries(self):
        """The fixed-capacity tensors and the device counts: no host read (what a captured step would consume)."""
        return {"input_ids": self.input_ids, "txt_mask_tgt": self.txt_mask_tgt, "txt_labels": self.txt_labels,
                "txt_mask_rows": self.txt_mask_rows, "c_v_masks": self.c_v_masks, "f_v_masks": self.f_v_masks,
                "feat_targets": self.feat_targets, "c_v_feats": self.c_v_feats, "f_v_feats": self.f_v_feats,
                "shuffled_orders": self.shuffled_orders, "targets": self.targets, "counts": self.counts}
