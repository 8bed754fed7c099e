"""Generates the WaveFlow shape fixtures tests/golden/wf/model_<name>.npz by running the UPSTREAM REFERENCE's model/waveflow.py (imported
through ref_shim) on the CPU, on deterministic inputs and parameters from fill.py.  Build container only.

    python tests/golden/make_golden_waveflow.py              # every case of fill.WF_SHAPE_FIXTURES (about a minute)
    python tests/golden/make_golden_waveflow.py wf128c ...   # single cases

The cases are the heights of the reference's dilation_dict that the fixtures of make_golden.py do not have (n_group 16, 32, 128) and
column counts past one 256-column block (wf8_long, wf64_long), each with the flip and with use_conv1x1=True (suffix c), n_group 128 also
with WN2D(bias=True) (wf128b); fill.WF_CONFIGS / fill.WF_SHAPES hold them.  The function that runs the reference is
make_golden.waveflow_fixture, the one that writes model_wf8.npz / model_wf64.npz: same contents (z, logdet, loss, dmel, x_inv, logdet_inv,
y_up in full, norm / head / max of every gradient, every invconv1x1 and bias gradient in full).  The fixtures live in their own
directory, next to (not among) the ones make_golden.py main() regenerates.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("WG_GOLDEN_OUT") or os.path.join(HERE, "wf")     # (tests regenerate into a scratch directory)
import fill                               # noqa: E402
from make_golden import waveflow_fixture  # noqa: E402


def main(names=None):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    for name in names or fill.WF_SHAPE_FIXTURES:
        assert name in fill.WF_SHAPE_FIXTURES, name
        waveflow_fixture(name, OUT)


if __name__ == "__main__":
    main(sys.argv[1:])
