"""sha256 of FusedAdam's results in every mode and memory layout (run on the GPU box):

    python tools/adam_digest.py      DGMR_LIB=<other build> for the other side of an A/B

The recipe of the optimiser's GPU tests (tests/adam_recipe.py: seven tensors, five steps, then swap_ema() and back) in the modes plain /
guarded / ema / guarded+ema, each on separately allocated tensors, on gradients that are views at odd element offsets into a flat
buffer, and on parameters that are such views.  One digest per (mode, layout) over every snapshot: p, exp_avg, exp_avg_sq, the
shadows, the guard's norm and coefficient.  Two builds of the library that claim the same bits must print the same twelve lines."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as g  # noqa: E402

if not os.environ.get("DGMR_LIB"):
    g.build()
import adam_recipe as R  # noqa: E402

for mode in R.MODES:
    for layout in R.LAYOUTS:
        h = hashlib.sha256()
        for shot in R.run(mode, layout):
            for t in shot:
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
        print(f"{mode:12s} {layout:12s} {h.hexdigest()}")
