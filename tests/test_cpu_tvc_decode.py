"""Incremental captioning decode (HeroForTvc.init_decode_state / decode_step, TvcGenerator(kv_cache=True)) on CPU tensors, where it
takes the PyTorch formulation of the step - keys and values kept per layer and grown by concatenation - against
tests/golden/case_tvc.npz and against the uncached formulation of the same module; and the host-side envelope query of the
one-row attention kernels.  The encoder has no CPU route, so the fixture's encoder outputs go in, as in tests/test_cpu_tvc.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, config_file, rel_err

Z = np.load(os.path.join(GOLDEN, "case_tvc.npz"))
DESC = json.loads(str(Z["desc"]))


@pytest.fixture(scope="module")
def built_lib():
    from hero_amd import build
    return build.build()


def _model():
    from hero_amd.model import HeroForTvc
    from hero_amd.utils.misc import set_dropout
    cfg = json.load(open(os.path.join(GOLDEN, "tiny_config.json")))
    cfg["d_config"] = DESC["d_config"]
    z = np.load(os.path.join(GOLDEN, "tiny_model.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("__")}
    sd.update({k[len("param."):]: torch.from_numpy(Z[k].astype(np.float32)) for k in Z.files if k.startswith("param.")})
    model = HeroForTvc.from_pretrained(config_file(cfg, "tiny_tvc.json"), sd, vfeat_dim=int(z["__vfeat__"]),
                                       max_frm_seq_len=int(z["__max_frm__"]))
    model.train()
    set_dropout(model, 0.0)
    return model


def _batch():
    return {k[len("out."):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("out.") and Z[k].dtype.kind != "U"}


def test_cached_decode_on_cpu_takes_the_pytorch_step_and_returns_the_fixture_ids():
    from hero_amd.model import TvcGenerator
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    state = model.init_decode_state(enc, b["cap_attn_mask"], 8)
    assert not state.fused and state.cache == [] and len(state.cross_k) == DESC["d_config"]["num_hidden_layers"]
    gen = TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"]), kv_cache=True)
    assert gen.greedy_decode(b, encoder_outputs=enc) == json.loads(str(Z["greedy"]))
    assert float(Z["greedy_margin"]) >= 1e-3                                     # no arg-max of the fixture is a near tie
    # the default is the uncached loop, and it gives the same ids
    assert not TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"])).kv_cache
    assert TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"])).greedy_decode(b, encoder_outputs=enc) == json.loads(str(Z["greedy"]))


def test_teacher_forced_step_scores_match_the_uncached_formulation():
    """Feeding the fixture's input ids position by position: the scores of step t against column t of the full decoder run of the
    same module (PyTorch ops on both sides) and against the reference's scores, at the project's fp32 gate rel_err < 2e-4."""
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    ids = b["cap_input_ids"]
    with torch.no_grad():
        full = model.decode(enc, b["cap_attn_mask"], ids, b["cap_pos_ids"], None, compute_loss=False)
    state = model.init_decode_state(enc, b["cap_attn_mask"], ids.shape[1])
    want = torch.from_numpy(Z["scores"])
    for t in range(ids.shape[1]):
        got = model.decode_step(state, ids[:, t])
        assert got.shape == full[:, t].shape and state.t == t + 1
        assert state.self_k[0].shape[1] == t + 1                                 # the keys grew by one row
        e_full, e_ref = rel_err(got, full[:, t]), rel_err(got, want[:, t])
        assert e_full < 2e-4 and e_ref < 2e-4, (t, e_full, e_ref)
    with pytest.raises(ValueError, match="decode step"):
        model.decode_step(state, ids[:, 0])                                      # past the state's max_step
    # the same buffers serve another batch of the same shape
    model.refill_decode_state(state, enc, b["cap_attn_mask"])
    assert state.t == 0 and rel_err(model.decode_step(state, ids[:, 0]), full[:, 0]) < 2e-4
    with pytest.raises(ValueError, match="decode state was made for"):
        model.refill_decode_state(state, enc[:, :-1], b["cap_attn_mask"][:, :-1])


def test_use_graph_without_kv_cache_raises():
    from hero_amd.model import TvcGenerator
    with pytest.raises(ValueError, match="kv_cache"):
        TvcGenerator(None, 8, 0, 2, use_graph=True)
    with pytest.raises(ValueError, match="kv_cache"):
        TvcGenerator(None, 8, 0, 2, kv_cache=False, use_graph=True)


def test_use_graph_on_cpu_tensors_raises():
    from hero_amd.model import TvcGenerator
    model, b, enc = _model(), _batch(), torch.from_numpy(Z["enc_out"])
    with pytest.raises(ValueError, match="kernels' route"):
        TvcGenerator(model, 8, DESC["bos"], int(Z["greedy_eos"]), kv_cache=True, use_graph=True).greedy_decode(b, encoder_outputs=enc)


def test_row_envelope_query_needs_no_gpu(built_lib):
    """hero_dec_attention_row_in_envelope answers on the host; hero_amd.tvc.in_envelope_row wraps it."""
    from hero_amd import _lib as Lb
    from hero_amd import tvc
    for dtype in (Lb.F32, Lb.BF16):
        assert Lb.lib().hero_dec_attention_row_in_envelope(dtype, 1) == 1 and Lb.lib().hero_dec_attention_row_in_envelope(dtype, 128) == 1
        assert Lb.lib().hero_dec_attention_row_in_envelope(dtype, 0) == 0 and Lb.lib().hero_dec_attention_row_in_envelope(dtype, 129) == 0
    assert Lb.lib().hero_dec_attention_row_in_envelope(7, 8) == 0
    for dtype in (torch.float32, torch.bfloat16):
        assert tvc.in_envelope_row(dtype, 1) and tvc.in_envelope_row(dtype, 128)
        assert not tvc.in_envelope_row(dtype, 0) and not tvc.in_envelope_row(dtype, 129)
    assert not tvc.in_envelope_row(torch.float16, 8)
