"""Which stages' first blocks run their projection shortcut fused into conv3 (net.shortcut_fusion), at 1, 8 and 64 frames per pass, and
the switches that turn it off.  Shapes only: meta tensors, no GPU."""
import importlib

import pytest
import torch


@pytest.fixture(scope="module")
def net_mod(pkg):
    return importlib.import_module("amos_slam_amd.mask.net")


@pytest.fixture(scope="module")
def trunk(net_mod):
    t = net_mod.ResNet50Trunk()
    t.fold_batch_norms()
    return t


def _fused_stages(net_mod, trunk, frames):
    """The stages (0 - 3) whose first block fuses, for the 550 x 550 network input (138 x 138 after the stem)."""
    c, h = 64, 138
    out = []
    for stage, layer in enumerate(trunk.layers):
        block = layer[0]
        s = block.downsample[0].stride[0]
        oh = (h - 1) // s + 1
        x = torch.empty((frames, c, h, h), device="meta")
        y = torch.empty((frames, block.conv3.in_channels, oh, oh), device="meta")
        if net_mod.shortcut_fusion(block, x, y):
            out.append(stage)
        c, h = block.conv3.out_channels, oh
    return out


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("AMOS_MASK_BOTTLENECK_FUSION", "AMOS_MASK_CONV1X1", "AMOS_GEMM_NARROW"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("frames, stages", [(64, [0, 1, 2, 3]), (8, [0, 1]), (1, [])])
def test_fused_stages_per_pass_size(net_mod, trunk, frames, stages):
    # 8 frames: stages 3 and 4 run 128 x 64 tiles (616 / 336 work-groups of 128 x 128 would be fewer than 1 024), which the fused
    # kernel does not; one frame: none of the stages has the 128 x 128 tiles
    assert _fused_stages(net_mod, trunk, frames) == stages


@pytest.mark.parametrize("env, value", [("AMOS_MASK_BOTTLENECK_FUSION", "0"), ("AMOS_MASK_CONV1X1", "1"), ("AMOS_MASK_CONV1X1", "0")])
def test_switches_turn_the_fusion_off(net_mod, trunk, monkeypatch, env, value):
    monkeypatch.setenv(env, value)
    assert _fused_stages(net_mod, trunk, 64) == []


def test_unfolded_and_cpu_blocks_do_not_fuse(net_mod, trunk):
    raw = net_mod.ResNet50Trunk()
    x = torch.empty((64, 64, 138, 138), device="meta")
    y = torch.empty((64, 64, 138, 138), device="meta")
    assert net_mod.shortcut_fusion(trunk.layers[0][0], x, y)
    assert not net_mod.shortcut_fusion(raw.layers[0][0], x, y)  # batch norms not folded
    assert not net_mod.shortcut_fusion(trunk.layers[0][1], torch.empty((64, 256, 138, 138), device="meta"), y)  # no projection
    assert not net_mod.shortcut_fusion(trunk.layers[0][0], torch.empty((64, 64, 138, 138)), torch.empty((64, 64, 138, 138)))  # CPU
