#!/usr/bin/env python3
"""Generate the YAMLs of the reference's Strip R-CNN config (configs/strip_rcnn_s_fpn_1x_dota_with_flip.py: StripRCNN on a StripNet_S backbone with a StripHead) under
tests/golden/configs/, with the helpers and the layout of gen_configs.py:

    python tests/golden/gen_configs_strip.py <reference checkout>

Settings only (model, optimizer, scheduler, name); no reference source text is stored."""
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_configs import OUT, SECTIONS, plain  # noqa: E402
from jdet_amd.config import Config  # noqa: E402  (gen_configs put the repository root on the path)

CONFIGS = ["configs/strip_rcnn_s_fpn_1x_dota_with_flip.py"]


if __name__ == "__main__":
    ref = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    for rel in CONFIGS:
        c = Config(os.path.join(ref, rel)).dump()
        path = os.path.join(OUT, os.path.splitext(os.path.basename(rel))[0] + ".yaml")
        with open(path, "w") as f:
            f.write("# %s of the reference, as Config reads it (tests/golden/gen_configs_strip.py)\n" % rel)
            yaml.safe_dump({k: plain(c[k]) for k in SECTIONS}, f, sort_keys=False, default_flow_style=None)
        print(path)
