"""CPU: host logic of the drop-in layer — config loading, registry surface, checkpoint key names, C-ABI exports."""
import ast
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import projects.mmdet3d_plugin  # noqa: F401  (registers everything, like plugin_dir= in the shipped configs)
from uni3detr_amd import native as nv
from uni3detr_amd.registry import (ATTENTION, BACKBONES, BBOX_ASSIGNERS, BBOX_CODERS, Config, DETECTORS, HEADS, LOSSES, MATCH_COST,
                                   MIDDLE_ENCODERS, NECKS, TRANSFORMER, TRANSFORMER_LAYER_SEQUENCE, build_model, to_config)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
# the six shipped configs (projects/configs/uni3detr/uni3detr_*.py) as Config.fromfile resolves them: per file its `_base_` list and
# the sections the tests read (oracle/make_golden.py gen_shipped_configs)
SHIPPED = ast.literal_eval(open(os.path.join(G, "shipped_configs.txt")).read())


def shipped(name):
    return Config(to_config(SHIPPED[name]["config"]))


def test_registry_surface():
    for reg, names in [(DETECTORS, ["Uni3DETR"]), (MIDDLE_ENCODERS, ["SparseEncoderHD"]), (BACKBONES, ["SECOND3D"]),
                       (NECKS, ["SECOND3DFPN"]), (HEADS, ["Uni3DETRHead"]), (TRANSFORMER, ["Uni3DETRTransformer"]),
                       (TRANSFORMER_LAYER_SEQUENCE, ["Uni3DETRTransformerDecoder"]), (ATTENTION, ["UniCrossAtten", "MultiheadAttention"]),
                       (BBOX_ASSIGNERS, ["HungarianAssigner3D"]), (MATCH_COST, ["BBox3DL1Cost", "IoU3DCost", "FocalLossCost"]),
                       (BBOX_CODERS, ["NMSFreeCoder"]), (LOSSES, ["SoftFocalLoss", "IoU3DLoss", "L1Loss"])]:
        for n in names:
            assert n in reg, (reg.name, n)


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "u3d_hip.h")).read()
    declared = set(re.findall(r"\b(u3d_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"u3d_stream"}
    lib = ctypes.CDLL(nv.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/u3d_hip.h but not exported"
    assert declared == set(nv.exported_symbols()), declared ^ set(nv.exported_symbols())
    assert lib.u3d_version() >= 1


# u3d_igemm_fwd_plan asked with STATS and n-major weights: (n_out_cap, cin, cout, kvol, has_nbr) -> (statistics partials, rows per
# partial), None = no kernel with a statistics epilogue serves the shape; rows 0 = one partial per wave of the direct-operand kernels.  Direct-operand row counts are
# small enough that the grid is bounded by the tiles, not by the CU count (256 assumed without a GPU, as the MI355X has).
STATS_LAYOUT = [
    # tests/test_sparse_gpu.py::test_conv_epilogue_bn_statistics_match_separate_pass
    (1200, 64, 64, 27, 1, (10, 128)), (1188, 128, 256, 27, 1, (10, 128)), (192000, 256, 256, 27, 1, (750, 256)),
    (3003, 32, 32, 27, 1, (64, 0)), (1200, 16, 32, 27, 1, (32, 0)), (1512, 64, 32, 27, 1, (64, 0)), (12240, 32, 16, 27, 1, (192, 0)),
    (60, 64, 16, 27, 1, (32, 0)), (12000, 512, 512, 27, 1, (63, 192)), (44640, 256, 256, 27, 1, (233, 192)),
    (40000, 512, 512, 27, 1, (209, 192)),
    # 256-column tiles at 127 / 128 workgroups, with and without a table
    (32512, 256, 256, 27, 1, (127, 256)), (32513, 256, 256, 27, 1, (170, 192)), (32512, 256, 256, 1, 0, (254, 128)),
    (32513, 256, 256, 1, 0, (128, 256)),
    # 256 x 128 eight-phase tiles: 159 / 160 workgroups, 47 / 48 k-tiles
    (40704, 128, 128, 27, 1, (318, 128)), (40705, 128, 128, 27, 1, (213, 192)), (48000, 64, 128, 47, 1, (375, 128)),
    (48000, 64, 128, 48, 1, (250, 192)),
    # 192-row tiles flip back to 256 rows (both eight-phase kernels); one offset: never 192 rows
    (49152, 256, 256, 27, 1, (256, 192)), (49153, 256, 256, 27, 1, (193, 256)), (49152, 128, 128, 27, 1, (256, 192)),
    (49153, 128, 128, 27, 1, (193, 256)), (49152, 256, 256, 1, 1, (192, 256)),
    # cout % 128 against cout % 256
    (48000, 128, 384, 27, 1, (250, 192)), (48000, 128, 512, 27, 1, (250, 192)), (12000, 512, 384, 27, 1, (94, 128)),
    (12000, 512, 512, 27, 1, (63, 192)),
    # no table
    (48000, 256, 256, 1, 0, (188, 256)), (12000, 512, 512, 1, 0, (94, 128)),
    # without a table the long-reduction rule does not apply, even at 3072 input channels: 128-row tiles
    (12000, 3072, 512, 1, 0, (94, 128)),
    # direct-operand shapes, 64 -> 64 (LDS-DMA), a 32 -> 64 statistics launch (none), not 27 offsets, empty outputs, cin % 64
    (12240, 16, 16, 27, 1, (192, 0)), (12240, 32, 32, 27, 1, (192, 0)), (12240, 64, 16, 27, 1, (192, 0)),
    (12240, 64, 32, 27, 1, (192, 0)), (12240, 64, 64, 27, 1, (96, 128)), (12240, 32, 64, 27, 1, None),
    (12240, 32, 32, 9, 1, None), (0, 32, 32, 27, 1, (0, 0)), (0, 64, 64, 27, 1, None), (1200, 48, 64, 27, 1, None),
    # the statistics launches of bench.py's workloads (sunrgbd bf16 / parity, kitti_3classes, scannet_large, nuscenes): smallest and
    # largest row count per shape
    (64000, 16, 16, 27, 1, (1024, 0)), (206938, 32, 64, 27, 1, None), (960000, 32, 64, 27, 1, None),
    (206938, 64, 64, 81, 1, (1617, 128)), (272384, 64, 64, 81, 1, (2128, 128)), (53947, 64, 128, 27, 1, (422, 128)),
    (363264, 64, 128, 27, 1, (2838, 128)), (53947, 64, 128, 81, 1, (211, 256)), (71680, 64, 128, 81, 1, (374, 192)),
    (192000, 128, 128, 9, 1, (1500, 128)), (704000, 128, 128, 9, 1, (5500, 128)), (192000, 128, 128, 27, 1, (750, 256)),
    (53947, 128, 128, 81, 1, (211, 256)), (71680, 128, 128, 81, 1, (374, 192)), (53947, 128, 256, 1, 0, (211, 256)),
    (704000, 128, 256, 1, 0, (2750, 256)), (53947, 128, 256, 3, 1, (211, 256)), (192000, 128, 256, 3, 1, (750, 256)),
    (70348, 128, 256, 27, 1, (367, 192)), (91648, 128, 256, 27, 1, (478, 192)), (192000, 256, 128, 9, 1, (1500, 128)),
    (704000, 256, 128, 9, 1, (5500, 128)), (192000, 256, 128, 27, 1, (750, 256)), (48000, 256, 256, 9, 1, (250, 192)),
    (176000, 256, 256, 9, 1, (688, 256)), (48000, 256, 256, 27, 1, (250, 192)), (704000, 256, 256, 27, 1, (2750, 256)),
    (192000, 256, 256, 81, 1, (750, 256)), (70348, 256, 512, 1, 0, (275, 256)), (91648, 256, 512, 1, 0, (358, 256)),
    (12000, 256, 512, 9, 1, (94, 128)), (44000, 256, 512, 9, 1, (230, 192)), (12000, 256, 512, 27, 1, (63, 192)),
    (384000, 512, 128, 9, 1, (1500, 256)), (96000, 512, 256, 9, 1, (500, 192)), (12000, 512, 512, 9, 1, (63, 192)),
    (44000, 512, 512, 9, 1, (230, 192)), (12000, 512, 512, 27, 1, (63, 192)),
]


def test_fwd_stats_layout_follows_the_dispatch():
    for n, cin, cout, kvol, has_nbr, want in STATS_LAYOUT:
        info = nv.FwdPlanInfo(partials=-1, rows_per_partial=-1)
        rc = nv.lib().u3d_igemm_fwd_plan(n, cin, cout, kvol, has_nbr, 1, nv.FWD_EPI["stats"], ctypes.byref(info))
        got = (info.partials, info.rows_per_partial) if rc == 0 else (None if rc == -2 else rc)
        assert got == want, ((n, cin, cout, kvol, has_nbr), got, want)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(nv, "_lib", None)
    monkeypatch.setattr(nv, "LIB_PATH", "/nonexistent/libu3d_hip.so")
    with pytest.raises(nv.U3DError):
        nv.lib()


@pytest.mark.parametrize("name", ["sunrgbd", "scannet", "scannet_large", "kitti_3classes", "kitti_car", "nuscenes"])
def test_shipped_configs_load_unchanged_and_build(name, tmp_path):
    # a config file laid out as the shipped one (projects/configs/uni3detr/, the same `_base_` paths into the absent mmdetection3d
    # configs/_base_/): Config.fromfile serves the bases from uni3detr_amd/configs/_base_/ and reproduces the shipped resolution
    ent = SHIPPED[name]
    d = tmp_path / "projects" / "configs" / "uni3detr"
    d.mkdir(parents=True)
    own = {k: v for k, v in ent["config"].items() if k in ("plugin", "plugin_dir", "model")}
    (d / f"uni3detr_{name}.py").write_text(f"_base_ = {ent['bases']!r}\n" + "".join(f"{k} = {v!r}\n" for k, v in own.items()))
    cfg = Config.fromfile(str(d / f"uni3detr_{name}.py"))
    assert cfg.model == ent["config"]["model"]
    assert cfg.model.type == "Uni3DETR" and cfg.plugin_dir == "projects/mmdet3d_plugin/"
    assert cfg.dist_params.backend == "nccl"            # came from the supplied _base_/default_runtime.py
    assert cfg.dist_params == ent["config"]["dist_params"]
    model = build_model(cfg.model)
    assert model.pts_bbox_head.num_query == cfg.model.pts_bbox_head.num_query
    cfg.merge_from_dict({"model.pts_bbox_head.num_query": 10})
    assert cfg.model.pts_bbox_head.num_query == 10


def test_builtin_sunrgbd_config_equals_shipped():
    from uni3detr_amd.configs.sunrgbd import model as mine
    ref = shipped("sunrgbd").model
    assert json.dumps(mine, sort_keys=True, default=list) == json.dumps(ref, sort_keys=True, default=list)
    m = build_model(mine)
    assert sum(p.numel() for p in m.parameters()) == 31707880


def test_head_state_dict_keys_match_reference_checkpoint_names():
    from uni3detr_amd.configs.sunrgbd import model as mine
    m = build_model(mine)
    z = np.load(os.path.join(G, "head_train_b2.npz"))
    mine_keys = {k: tuple(v.shape) for k, v in m.pts_bbox_head.state_dict().items()}
    ref_keys = {str(k): tuple(int(s) for s in str(shp).split(",")) if str(shp) else () for k, shp in zip(z["sd_names"], z["sd_shapes"])}
    assert mine_keys == ref_keys
    sd = m.state_dict()
    for k in ["pts_middle_encoder.conv_input.0.weight", "pts_middle_encoder.encoder_layers.encoder_layer1.0.conv1.weight",
              "pts_middle_encoder.encoder_layers.encoder_layer1.2.0.weight", "pts_middle_encoder.encoder_layers.encoder_layer4.1.bn2.running_var",
              "pts_middle_encoder.conv_out.1.num_batches_tracked", "pts_backbone.blocks.2.15.weight", "pts_backbone.blocks.0.16.bias",
              "pts_neck.deblocks.1.0.weight", "pts_neck.extra_blocks.6.weight", "pts_neck.extra_blocks.7.running_mean",
              "pts_bbox_head.transformer.decoder.layers.0.attentions.1.output_proj.weight", "pts_bbox_head.code_weights"]:
        assert k in sd, k
    assert tuple(sd["pts_middle_encoder.encoder_layers.encoder_layer3.2.0.weight"].shape) == (3, 3, 3, 64, 128)
    assert tuple(sd["pts_neck.deblocks.2.0.weight"].shape) == (512, 256, 1, 4, 4)


@pytest.mark.parametrize("name", ["scannet_large", "kitti_3classes", "nuscenes", "sunrgbd"])
def test_builtin_variants_equal_shipped_configs(name):
    from uni3detr_amd.configs import variants
    ref = shipped(name).model
    assert json.dumps(getattr(variants, name), sort_keys=True, default=list) == json.dumps(ref, sort_keys=True, default=list)


def test_hot_kernels_keep_their_register_budget(tmp_path):
    """Guard against silent register-allocation regressions in the built library (one refactor of the LDS-DMA kernels' epilogue made
    the 256x256 kernel spill and halved the 128x128 kernel's occupancy: 25.4 -> 27.5 ms per step with every test green).  Reads the
    gfx950 code objects' metadata: no scratch in the implicit-GEMM kernels; the 256x256 tiles fit two waves per SIMD (<= 256 VGPRs),
    the 128x128 forward tile two workgroups per CU (<= 256 VGPR + AGPR)."""
    import re
    import shutil
    import subprocess
    from uni3detr_amd import native as nv
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf) and os.path.exists(nv.LIB_PATH)):
        pytest.skip("ROCm LLVM tools or the built library are not available")
    lib = shutil.copy(nv.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    kernels = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
            kernels[name.group(1)] = dict(agpr=int(blk.split()[0]), vgpr=get("vgpr_count"), scratch=get("private_segment_fixed_size"))
    find = lambda sub: [v for k, v in kernels.items() if sub in k]
    assert len(kernels) > 50
    for sub in ("k_igemm_glds_256x256", "k_igemm_glds_128x128", "k_igemm_glds_128x64", "k_igemm_wgrad_glds_256", "k_igemm_wgrad_glds_128",
                "k_igemm_glds8_256x256", "k_igemm_glds8_256x256_f32o", "k_igemm_glds8_256x128_f32o"):
        ks = find(sub)
        assert ks, sub
        assert all(k["scratch"] == 0 for k in ks), (sub, ks)
    assert all(k["vgpr"] <= 256 and k["agpr"] == 0 for k in find("k_igemm_glds_256x256"))
    assert all(k["vgpr"] + k["agpr"] <= 256 for k in find("k_igemm_glds_128x128"))


def test_nms_free_coder_decode_matches_reference_golden():
    """NMSFreeCoder.decode vs the reference file's own output (tests/golden/coder_decode.npz, generated by oracle/make_golden.py from
    core/bbox/coders/nms_free_coder.py:42-136): top-k over query x class, score^alpha * iou^(1-alpha), score and centre-range masks."""
    import numpy as np
    from uni3detr_amd.plugin.bbox import NMSFreeCoder
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "coder_decode.npz"))
    preds = dict(all_cls_scores=torch.from_numpy(z["cls"]), all_bbox_preds=torch.from_numpy(z["box"]), all_iou_preds=torch.from_numpy(z["iou"]))
    si = 0
    while f"s{si}_cfg" in z:
        c = z[f"s{si}_cfg"]
        coder = NMSFreeCoder(pc_range=list(z["pc_range"]), voxel_size=[0.02] * 3, post_center_range=[float(v) for v in c[3:9]], max_num=int(c[2]),
                             score_threshold=None if c[1] < 0 else float(c[1]), alpha=float(c[0]), num_classes=10)
        res = coder.decode(preds)
        for b, r in enumerate(res):
            assert r["labels"].numpy().tolist() == z[f"s{si}_b{b}_labels"].tolist(), (si, b)
            for k in ("bboxes", "scores", "ious"):
                ref = z[f"s{si}_b{b}_{k}"]
                assert r[k].shape == ref.shape and np.abs(r[k].numpy() - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), (si, b, k)
        si += 1
    assert si == 3


@pytest.mark.parametrize("spconv2", [False, True])
def test_checkpoint_round_trip_incl_spconv2_layout(tmp_path, spconv2):
    """save -> load (ref: extra_tools/test.py:197) restores every tensor bit for bit, also from a checkpoint whose sparse-conv weights
    are in the spconv 2.x layout [Cout,kD,kH,kW,Cin] and whose keys carry DDP's 'module.' prefix; a wrong shape is refused (identical
    detections from the reloaded model: tests/test_postproc_gpu.py)."""
    from uni3detr_amd.checkpoint import load_checkpoint, save_checkpoint
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    torch.manual_seed(1)
    a = build_model(copy.deepcopy(MODEL_CFG))
    path = str(tmp_path / "ck.pth")
    ck = save_checkpoint(a, path, meta=dict(epoch=3), to_spconv2=spconv2)
    if spconv2:
        w = ck["state_dict"]["pts_middle_encoder.conv_input.0.weight"]
        assert w.shape[0] == a.state_dict()["pts_middle_encoder.conv_input.0.weight"].shape[-1]      # Cout first
        ck["state_dict"] = {"module." + k: v for k, v in ck["state_dict"].items()}
        torch.save(ck, path)
    torch.manual_seed(2)
    b = build_model(copy.deepcopy(MODEL_CFG))
    out = load_checkpoint(b, path)
    assert out["meta"]["epoch"] == 3
    assert bool(out["meta"]["converted_sparse_weights"]) == spconv2
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    bad = {k: v for k, v in sa.items()}
    bad["pts_bbox_head.tgt_embed.weight"] = torch.zeros(5, 5)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        load_checkpoint(b, dict(state_dict=bad))


class _Evil:
    """An object whose unpickling would run code (what a hostile checkpoint looks like)."""
    def __reduce__(self):
        return (os.path.join, ("a", "b"))


def test_checkpoint_with_python_objects_needs_explicit_trust(tmp_path, monkeypatch):
    """The tensors-only unpickler is the default; a file it rejects is loaded with the full (code-executing) unpickler ONLY on an
    explicit opt-in, and a missing file is an I/O error, not a reason to try the unsafe path."""
    from uni3detr_amd.checkpoint import load_checkpoint
    from uni3detr_amd.configs.sunrgbd import model as MODEL_CFG
    m = build_model(copy.deepcopy(MODEL_CFG))
    path = str(tmp_path / "evil.pth")
    torch.save({"meta": {"obj": _Evil()}, "state_dict": {k: v for k, v in m.state_dict().items()}}, path)
    monkeypatch.delenv("U3D_TRUST_CHECKPOINTS", raising=False)
    with pytest.raises(RuntimeError, match="trusted=True"):
        load_checkpoint(m, path)
    assert load_checkpoint(m, path, trusted=True)["meta"]["obj"] == os.path.join("a", "b")
    with pytest.raises(FileNotFoundError):
        load_checkpoint(m, str(tmp_path / "absent.pth"))


def test_unselected_registry_names_match_reference_goldens():
    """RDIoULoss / RDIoUCost / SoftFocalLossCost / get_rdiou (no shipped config selects them) against vectors produced by the reference's
    own files (oracle/make_golden.py gen_extra); AxisAlignedIoU3DCost / RotatedIoU3DCost build from the registry."""
    import numpy as np
    import torch
    from uni3detr_amd.plugin import extra_costs as X
    from uni3detr_amd.registry import LOSSES, MATCH_COST
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "extra_costs.npz"))
    t = lambda k: torch.from_numpy(z[k])
    u, r = X.get_rdiou(t("p").unsqueeze(1), t("g").unsqueeze(0))
    assert torch.allclose(u, t("u"), rtol=1e-5, atol=1e-6) and torch.allclose(r, t("rdiou"), rtol=1e-5, atol=1e-7)
    cost = MATCH_COST.build(dict(type="RDIoUCost", weight=1.7))(t("p"), t("g"))
    assert torch.allclose(cost, t("rdiou_cost"), rtol=1e-5, atol=1e-6)
    sfc = MATCH_COST.build(dict(type="SoftFocalLossCost", weight=2.0))(t("cls"), t("labels"), t("iou"))
    assert torch.allclose(sfc, t("soft_focal_cost"), rtol=1e-5, atol=1e-6)
    a = t("a").requires_grad_(True)
    loss = LOSSES.build(dict(type="RDIoULoss", loss_weight=1.2))(a, t("b"), t("w"), avg_factor=5.0)
    assert abs(float(loss) - float(z["rdiou_loss"])) <= 1e-5 * abs(float(z["rdiou_loss"]))
    loss.backward()
    assert torch.allclose(a.grad, t("rdiou_loss_grad"), rtol=1e-4, atol=1e-6)
    # axis-aligned IoU cost: closed form on unit cubes shifted by half an edge -> IoU = 0.5 / 1.5
    aa = MATCH_COST.build(dict(type="AxisAlignedIoU3DCost", weight=2.0))
    b0 = torch.tensor([[0.0, 0, 0, 1, 1, 1]])
    b1 = torch.tensor([[0.5, 0, 0, 1.5, 1, 1], [2.0, 2, 2, 3, 3, 3]])
    assert torch.allclose(aa(b0, b1), torch.tensor([[-2.0 / 3.0, 0.0]]), atol=1e-6)
    assert MATCH_COST.build(dict(type="RotatedIoU3DCost", weight=1.0)).weight == 1.0


def test_restated_pipelines_equal_the_shipped_config_files():
    from uni3detr_amd.configs import pipelines as P
    assert len(SHIPPED) == len(P.SHIPPED) == 6
    for name in sorted(SHIPPED):
        cfg = shipped(name)
        for key in ("train_pipeline", "test_pipeline"):
            ref, ours = getattr(cfg, key), P.SHIPPED[name][key]
            assert [e["type"] for e in ref] == [e["type"] for e in ours], (name, key)
            for r, o in zip(ref, ours):
                for a, v in o.items():
                    assert list(r[a]) == list(v) if isinstance(v, (list, tuple)) else r[a] == v, (name, key, a)
