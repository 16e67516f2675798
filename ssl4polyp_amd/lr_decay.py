"""Layer-wise learning-rate decay for the MAE fine-tune recipe: the parameter groups of mae/util/lr_decay.py:15-76 (after BEiT /
ELECTRA), restated.  A ViT of `depth` blocks has depth + 2 layer ids: 0 = everything in front of the first block (cls_token,
pos_embed, patch_embed.*), i + 1 = blocks.i.*, depth + 1 = whatever sits behind the stack (norm / fc_norm, head).  Layer id l
trains at lr_scale = layer_decay ** (depth + 1 - l); train.adjust_learning_rate multiplies the scheduled lr by it and
optim.FusedAdamW takes the groups as they are.  tests/golden/layer_decay.json pins names, order and numbers to the reference's own
function."""
from __future__ import annotations

from typing import Dict, Iterable, List


def get_layer_id_for_vit(name: str, num_layers: int) -> int:
    """lr_decay.py:64-76."""
    if name in ("cls_token", "pos_embed"):
        return 0
    if name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay: float = 0.05, no_weight_decay_list: Iterable[str] = (), layer_decay: float = 0.75,
                     with_names: bool = False) -> List[Dict]:
    """lr_decay.py:15-61: one group per (layer id, decay / no_decay) in first-appearance order over model.named_parameters(),
    frozen parameters skipped; weight_decay 0 for 1-D parameters and the names of no_weight_decay_list.  Each group holds
    "lr_scale", "weight_decay", "params" -- and with_names=True also "name" (`layer_<id>_<decay|no_decay>`) and "param_names",
    which the reference keeps in a second dict it only prints."""
    no_weight_decay_list = set(no_weight_decay_list)
    num_layers = len(model.blocks) + 1
    layer_scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    groups: Dict[str, Dict] = {}
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.ndim == 1 or n in no_weight_decay_list:
            g_decay, this_decay = "no_decay", 0.0
        else:
            g_decay, this_decay = "decay", weight_decay
        layer_id = get_layer_id_for_vit(n, num_layers)
        group_name = "layer_%d_%s" % (layer_id, g_decay)
        if group_name not in groups:
            groups[group_name] = {"lr_scale": layer_scales[layer_id], "weight_decay": this_decay, "params": []}
            if with_names:
                groups[group_name].update(name=group_name, param_names=[])
        groups[group_name]["params"].append(p)
        if with_names:
            groups[group_name]["param_names"].append(n)
    return list(groups.values())
