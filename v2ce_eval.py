#!/usr/bin/env python3
"""Command line of the stage-2 score (the reference's ``train/scripts/stage2/stage2_metrics.py``): frames -> voxels
-> each sampler's events, scored against a recording's GT events; the implementation lives in
``v2ce-toolbox_amd/stage2_metrics.py``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from v2ce_toolbox_amd.stage2_metrics import main  # noqa: E402

if __name__ == "__main__":
    main()
