"""Writes tests/golden/layer_decay.json by running the reference's own layer-decay grouping
  param_groups_lrd / get_layer_id_for_vit   loaded from <reference>/src/ssl4polyp/models/mae/util/lr_decay.py by file path
on a CPU stand-in module that has the parameter names, order and dimensionalities of mae/models_vit.py's VisionTransformer (timm
0.4.12: cls_token, pos_embed, patch_embed.proj.*, blocks.<i>.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}.*, norm.*, head.*;
with global_pool fc_norm.* is registered behind head and norm is deleted) at a width of 8: the grouping reads names, ndim and
requires_grad only.  Cases: depth 12 and 32, with and without global_pool, everything trainable / some parameters frozen (pos_embed,
patch_embed.proj.bias, all of blocks.0, blocks.3.attn.qkv.weight, head.bias), weight_decay 0.05, layer_decay 0.75 and 0.65; the
no_weight_decay list is timm's {'pos_embed', 'cls_token'}.  Only group names, parameter names and numbers are stored: the group name
is the reference's own `layer_<id>_<decay|no_decay>` (it keeps them in a dict it does not return: rebuilt here from its
get_layer_id_for_vit and the group's weight_decay rule).

Usage: python tests/golden/make_layer_decay_fixture.py <reference checkout>"""
import importlib.util
import json
import os
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
NO_WEIGHT_DECAY = ["pos_embed", "cls_token"]
FROZEN = ["pos_embed", "patch_embed.proj.bias", "blocks.0.", "blocks.3.attn.qkv.weight", "head.bias"]
CASES = [(12, False, False, 0.75), (12, True, False, 0.75), (12, True, True, 0.65), (32, True, False, 0.75), (32, False, True, 0.75)]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Attn(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.qkv = nn.Linear(d, 3 * d)
        self.proj = nn.Linear(d, d)


class _Mlp(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.fc1 = nn.Linear(d, 4 * d)
        self.fc2 = nn.Linear(4 * d, d)


class _Block(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.norm1 = nn.LayerNorm(d)
        self.attn = _Attn(d)
        self.norm2 = nn.LayerNorm(d)
        self.mlp = _Mlp(d)


class _PatchEmbed(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.proj = nn.Conv2d(3, d, kernel_size=2, stride=2)


class StandIn(nn.Module):
    def __init__(self, depth, global_pool, d=8):
        super().__init__()
        self.patch_embed = _PatchEmbed(d)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, d))
        self.pos_embed = nn.Parameter(torch.zeros(1, 5, d))
        self.blocks = nn.Sequential(*[_Block(d) for _ in range(depth)])
        self.norm = nn.LayerNorm(d)
        self.head = nn.Linear(d, 3)
        if global_pool:
            self.fc_norm = nn.LayerNorm(d)
            del self.norm


def main(reference):
    ref = _load(os.path.join(reference, "src", "ssl4polyp", "models", "mae", "util", "lr_decay.py"), "ref_lr_decay")
    cases = []
    for depth, global_pool, freeze, layer_decay in CASES:
        model = StandIn(depth, global_pool)
        frozen = []
        if freeze:
            for n, p in model.named_parameters():
                if any(n == f or (f.endswith(".") and n.startswith(f)) for f in FROZEN):
                    p.requires_grad_(False)
                    frozen.append(n)
        names = {id(p): n for n, p in model.named_parameters()}
        groups = []
        for g in ref.param_groups_lrd(model, 0.05, no_weight_decay_list=NO_WEIGHT_DECAY, layer_decay=layer_decay):
            pn = [names[id(p)] for p in g["params"]]
            p0 = g["params"][0]
            decay = "no_decay" if (p0.ndim == 1 or pn[0] in NO_WEIGHT_DECAY) else "decay"
            groups.append({"name": "layer_%d_%s" % (ref.get_layer_id_for_vit(pn[0], depth + 1), decay), "lr_scale": g["lr_scale"],
                           "weight_decay": g["weight_decay"], "params": pn})
        cases.append({"depth": depth, "global_pool": global_pool, "frozen": frozen, "weight_decay": 0.05, "layer_decay": layer_decay,
                      "no_weight_decay": NO_WEIGHT_DECAY, "all_names": [n for n, _ in model.named_parameters()], "groups": groups})
    path = os.path.join(HERE, "layer_decay.json")
    with open(path, "w") as fh:
        json.dump({"cases": cases}, fh, indent=1)
    print(path, os.path.getsize(path), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
