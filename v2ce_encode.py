#!/usr/bin/env python3
"""Command line of the event -> grid encoders (the reference's ``train/scripts/utils/events_utils.py``): an events file,
split per frame pair, as signed, split or statistics voxel grids; the implementation lives in
``v2ce-toolbox_amd/event_grids.py``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from v2ce_toolbox_amd.event_grids import main  # noqa: E402

if __name__ == "__main__":
    main()
