#!/usr/bin/env python3
"""Generate tests/golden/configs/*.yaml: the settings of the four config files BASELINE.json names, as `Config` reads
them from the reference checkout (`_base_` files merged), so that the config tests need no checkout.

    python tests/golden/gen_configs.py <reference checkout>

Only the sections the tests build are kept (model, optimizer, scheduler) plus `name`; tuples are written as lists
(YAML has no tuples).  The fixtures are data: no reference source text is stored."""
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jdet_amd.config import Config  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CONFIGS = ["configs/s2anet/s2anet_r50_fpn_1x_dota.py",
           "configs/rotated_retinanet/rotated_retinanet_obb_r50_fpn_1x_dota.py",
           "configs/oriented_rcnn_r50_fpn_1x_dota_with_flip.py",
           "configs/faster_rcnn_RoITrans_r50_fpn_1x_dota.py"]
SECTIONS = ("name", "model", "optimizer", "scheduler")


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


if __name__ == "__main__":
    ref = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    for rel in CONFIGS:
        c = Config(os.path.join(ref, rel)).dump()
        path = os.path.join(OUT, os.path.splitext(os.path.basename(rel))[0] + ".yaml")
        with open(path, "w") as f:
            f.write("# %s of the reference, as Config reads it (tests/golden/gen_configs.py)\n" % rel)
            yaml.safe_dump({k: plain(c[k]) for k in SECTIONS}, f, sort_keys=False, default_flow_style=None)
        print(path)
