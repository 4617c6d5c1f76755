#!/usr/bin/env python3
"""Command line of the head fit: frames and a recording's GT events -> a state_dict whose ``UNet.pred`` is fitted to the
recording (``v2ce.py -m tuned.pt`` loads it) and the per-step loss history; the implementation lives in
``v2ce-toolbox_amd/finetune.py``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from v2ce_toolbox_amd.finetune import main  # noqa: E402

if __name__ == "__main__":
    main()
