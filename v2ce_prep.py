#!/usr/bin/env python3
"""Command line of the recording-side preparation (the reference's ``train/scripts/utils/physical_att.py`` as
``train/scripts/tools/gen_phy_att.py`` runs it): a clip and its events as physical-attention maps and log-frame residuals,
one per frame pair; the implementation lives in ``v2ce-toolbox_amd/physical_att.py``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from v2ce_toolbox_amd.physical_att import main  # noqa: E402

if __name__ == "__main__":
    main()
