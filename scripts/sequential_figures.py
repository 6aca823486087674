"""640x480, 20 synthetic frames: the ground-truth-initialised protocol beside the sequential one, both motions, on a
random-walk and on a constant-twist sequence (NOTES.md, "Sequential localisation").  One JSON line per configuration."""
import json
import os
import pathlib
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsplatloc_amd.data import Parser  # noqa: E402
from gsplatloc_amd.eval import evaluate_room  # noqa: E402
from gsplatloc_amd.synthetic import write_replica_constant_twist, write_replica_sequence  # noqa: E402

W, H, n = 640, 480, 20
for name, writer in (("random_walk", write_replica_sequence), ("constant_twist", write_replica_constant_twist)):
    root = pathlib.Path(tempfile.mkdtemp())
    writer(root, W, H, n)
    for kw in ({}, {"sequential": True, "motion": "hold"}, {"sequential": True, "motion": "constant_velocity"}):
        for _ in range(2):  # the second pass has every buffer warm
            r = evaluate_room(Parser("Replica", "room0", normalize=True, input_folder=str(root)), 2000, None, **kw)
        print("SEQ_FIG " + json.dumps({"sequence": name, **kw, **r}), flush=True)
