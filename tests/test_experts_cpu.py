"""Expert-form blobs on the host: conversion without a system, the pinned merge, the routing
coefficients from the blob, and how ``resolve_weights`` finds such a set.  The device side is tests/test_gpu_experts.py."""
import importlib

import numpy as np
import pytest
import torch

from pdb2reaction_amd import weights as W

CK = importlib.import_module("pdb2reaction_amd.checkpoint")

CONFIG = {"model": "escnmd_backbone", "sphere_channels": 128, "hidden_channels": 128, "edge_channels": 128, "lmax": 2, "mmax": 2,
          "num_layers": 4, "num_distance_basis": 64, "distance_function": "gaussian", "norm_type": "rms_norm_sh", "act_type": "gate",
          "ff_type": "spectral", "chg_spin_emb_type": "rand_emb", "cutoff": 6.0, "max_neighbors": 300, "max_num_elements": 100,
          "otf_graph": True, "direct_forces": False, "regress_stress": False, "always_use_pbc": False,
          "dataset_list": ["oc20", "omol", "omat", "odac", "omc"], "num_experts": 4, "use_dataset_embedding": True}


def fake_state(n_exp=4):
    """A fairchem-style state dict (``backbone.`` prefix, ``.weights`` expert stacks, routing network), float32 tensors."""
    ws = W.make_synthetic_experts(max(n_exp, 1), seed=3)
    state = {}
    for name, arr in ws.items():
        if name in ("normalizer.rmsd", "element_refs"):
            continue
        if name in W.EXPERT_WEIGHT_NAMES:
            a = np.asarray(arr) if n_exp >= 1 else np.zeros((0,) + np.asarray(arr).shape[1:], np.float32)
            state["backbone." + name[:-len(".weight")] + ".weights"] = torch.tensor(a)
        else:
            state["backbone." + name] = torch.tensor(np.asarray(arr))
    extra = {"normalizer.rmsd": ws["normalizer.rmsd"], "element_refs": ws["element_refs"]}
    return state, extra, ws


def test_convert_experts_round_trip_and_refusals():
    state, extra, ws = fake_state()
    blob = CK.convert_experts(state, extra=extra, model_config=CONFIG)
    back = W.unpack_blob(blob)
    assert back.meta["experts"] == 4 and "merged_for" not in back.meta and back.meta["model"]["cutoff"] == 6.0
    assert set(back) == set(ws)
    for k in ws:
        assert back[k].dtype == np.float32 and np.array_equal(back[k], ws[k]), k
    assert back[W.EXPERT_WEIGHT_NAMES[0]].shape == (4, 640, 768) and W.expert_count(back) == 4
    assert W.COMPOSITION_KEY in back and "routing_mlp.2.bias" in back
    assert W.variant_of(back)["ff_type"] == "spectral"
    assert W.pack_blob(back) == blob                                        # a weight set in expert form packs to the same blob
    small = W.unpack_blob(blob, skip=W.EXPERT_WEIGHT_NAMES)
    assert set(small) == set(ws) - set(W.EXPERT_WEIGHT_NAMES) and small.meta == back.meta
    with pytest.raises(ValueError, match="no coefficients"):
        CK.convert_experts(state, extra=extra, model_config=CONFIG, coefficients=np.ones(4))
    # mixed: one of the 24 already merged
    mixed = dict(state)
    key = "backbone." + W.EXPERT_WEIGHT_NAMES[5][:-len(".weight")]
    mixed[key + ".weight"] = mixed.pop(key + ".weights")[0]
    with pytest.raises(CK.UnsupportedCheckpoint, match="23 of the 24"):
        CK.convert_experts(mixed, extra=extra, model_config=CONFIG)
    mw = W.WeightSet(back, meta=back.meta)
    mw[W.EXPERT_WEIGHT_NAMES[5]] = back[W.EXPERT_WEIGHT_NAMES[5]][0]
    with pytest.raises(ValueError, match="23 of the 24"):
        W.pack_blob(mw)
    # a stack on a tensor that is not one of the SO(2) weights
    other = dict(state)
    other["backbone.mix_csd.weights"] = torch.stack([other.pop("backbone.mix_csd.weight")] * 4)
    with pytest.raises(CK.UnsupportedCheckpoint, match=r"mix_csd\.weight"):
        CK.convert_experts(other, extra=extra, model_config=CONFIG)
    # expert counts outside 1..64
    with pytest.raises(CK.UnsupportedCheckpoint, match="0 experts"):
        CK.convert_experts(fake_state(0)[0], extra=extra, model_config=CONFIG)
    many = {k: (torch.zeros((65,) + tuple(v.shape[1:])) if k.endswith(".weights") else v) for k, v in state.items()}
    with pytest.raises(CK.UnsupportedCheckpoint, match="65 experts"):
        CK.convert_experts(many, extra=extra, model_config=CONFIG)
    # no routing network, no experts at all
    with pytest.raises(KeyError, match="routing network"):
        CK.convert_experts({k: v for k, v in state.items() if "routing_mlp" not in k}, extra=extra, model_config=CONFIG)
    merged_state = {(k[:-1] if k.endswith(".weights") else k): (v[0] if k.endswith(".weights") else v) for k, v in state.items()}
    with pytest.raises(ValueError, match="no expert stacks"):
        CK.convert_experts(merged_state, extra=extra, model_config=CONFIG)


def test_merge_mole_ordered_is_the_pinned_loop():
    rng = np.random.default_rng(0)
    ex = rng.standard_normal((5, 3, 7)).astype(np.float32)
    al = rng.random(5)
    want = np.empty((3, 7), np.float32)
    for i in range(3):
        for j in range(7):
            s = 0.0
            for k in range(5):
                s = s + float(al[k]) * float(ex[k, i, j])
            want[i, j] = np.float32(s)
    got = CK.merge_mole_ordered(ex, al)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # summation ORDER decides the float32 result.  In order: 1 + 2^-24, then twice + 2^-53 -- half a float64 ulp each time, a tie that
    # goes to the even neighbour, i.e. is lost -- leaves 1 + 2^-24, the float32 tie, which rounds to even = 1.0f.  Reversed: 2^-53 + 2^-53
    # = 2^-52 survives, the sum is 1 + 2^-24 + 2^-52 exactly, just above the tie, and rounds up.  A tensordot may do either.
    e = np.array([1.0, 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], np.float32).reshape(4, 1)
    up = np.float32(1.0) + np.float32(2.0 ** -23)
    assert CK.merge_mole_ordered(e, [1.0] * 4)[0] == np.float32(1.0)
    assert CK.merge_mole_ordered(e[::-1], [1.0] * 4)[0] == up
    # and it differs from nothing else: merge_mole is as it was, to float64 accuracy the same sum
    assert CK.merge_mole(ex, al).dtype == np.float64
    np.testing.assert_allclose(CK.merge_mole(ex, al), got, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="experts but"):
        CK.merge_mole_ordered(ex, al[:-1])
    # the opt-in keyword of from_state_dict / convert selects it
    state, extra, ws = fake_state()
    rename = lambda n: None if W.is_routing_tensor(n) else n                  # noqa: E731
    p_ord = CK.from_state_dict(state, coefficients=al[:4], extra=extra, rename=rename, ordered_merge=True)
    p_blas = CK.from_state_dict(state, coefficients=al[:4], extra=extra, rename=rename)
    key = W.EXPERT_WEIGHT_NAMES[0]
    assert np.array_equal(p_ord[key], CK.merge_mole_ordered(ws[key], al[:4]))
    assert np.array_equal(p_blas[key], CK.merge_mole(ws[key], al[:4]).astype(np.float32))
    assert np.array_equal(CK.merge_expert_set(ws, al[:4])[key], p_ord[key])


def test_expert_coefficients_from_the_blob():
    state, extra, _ = fake_state()
    back = W.unpack_blob(CK.convert_experts(state, extra=extra, model_config=CONFIG))
    for z, q, s, t in (([8, 1, 1, 6, 1, 1, 1, 7], 0, 1, "omol"), ([26, 8, 8], -2, 3, "omat")):
        a = CK.expert_coefficients(back, z, q, s, t)
        assert a.shape == (4,) and a.dtype == np.float64 and abs(a.sum() - 1.0) < 1e-14
        np.testing.assert_allclose(a, CK.mole_coefficients(state, z, q, s, t), rtol=1e-12, atol=0)
    assert np.abs(CK.expert_coefficients(back, [8, 1, 1], 0, 1, "omol") - CK.expert_coefficients(back, [8, 1, 1], 1, 2, "omol")).max() > 1e-6


def test_resolve_weights_takes_expert_blobs_and_checkpoints(tmp_path, monkeypatch):
    U = importlib.import_module("pdb2reaction_amd.uma_pysis")
    state, extra, ws = fake_state()
    blob = CK.convert_experts(state, extra=extra, model_config=CONFIG)
    p = tmp_path / "uma-x.umxw"
    p.write_bytes(blob)
    got = U.resolve_weights(str(p))
    assert got.meta["experts"] == 4 and W.expert_count(got) == 4
    ck = tmp_path / "uma-y.pt"
    torch.save({"config": {"model": {"backbone": CONFIG}}, "state_dict": state,
                "normalizer.rmsd": torch.tensor(extra["normalizer.rmsd"]), "element_refs": torch.tensor(extra["element_refs"])}, str(ck))
    monkeypatch.setenv("UMX_WEIGHTS_DIR", str(tmp_path))
    for model in (str(ck), "uma-y"):
        via = U.resolve_weights(model)
        assert via.meta["experts"] == 4 and set(via) == set(got)
        assert all(np.array_equal(via[k], got[k]) for k in got)
    for w in (got, via):                                                     # one set, any system
        W.check_merged_for(w, [1, 1, 8], 0, 1, "omol")
        W.check_merged_for(w, [6, 1, 1, 1, 1], 1, 2, "omat")
    junk = tmp_path / "junk.pt"
    junk.write_bytes(b"not a checkpoint at all")
    with pytest.raises(CK.UnsupportedCheckpoint, match="weights_only=True"):
        U.resolve_weights(str(junk))


def test_new_kernels_are_in_the_library_and_the_digest():
    """The merge kernel keeps product and sum apart (no v_fma_f64 anywhere in it), and the new header is part of the source digest."""
    import os
    import re

    from pdb2reaction_amd import build

    assert any(os.path.basename(d) == "umx_experts.h" for d in build.dependencies())
    text = build.device_disassembly()
    bodies = {k: re.search(r"^[0-9a-f]+ <[^>]*%s[^>]*>:\n(.*?)(?=^[0-9a-f]+ <|\Z)" % k, text, flags=re.M | re.S) for k in ("k_mole_merge", "k_pack_planes")}
    assert all(bodies.values()), "the expert kernels are not in the gfx950 code object"
    merge = bodies["k_mole_merge"].group(1)
    assert "v_mul_f64" in merge and "v_add_f64" in merge and "v_cvt_f32_f64" in merge
    assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b", merge)
    assert build.check_no_packed_fp32() > 0
