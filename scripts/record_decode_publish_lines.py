"""Record tests/golden/decode_publish_lines.npz: logits, latents and appended K / V rows of the cases of
tests/test_gpu_decode_publish_lines.py, from the library that GENVC_HIP_LIB names.  The committed fixture comes from the build of the commit
BEFORE the one-stream step's whole-line publishes (profiles/decode_publish_lines.md), so the test holds later changes of how a hand-off
granule is stored to those bits.  Needs an MI355X.

    GENVC_HIP_LIB=/path/to/libgenvc_hip.so python scripts/record_decode_publish_lines.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import test_gpu_decode_publish_lines as T
from genvc_amd import _lib

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
print(f"library: {_lib.LIB_PATH}")
data = T.run_all()
np.savez_compressed(out, **data)
print(f"{out}: {len(data)} arrays, {os.path.getsize(out)} bytes")
for k in sorted(data):
    print(f"  {k:28s} {str(data[k].dtype):8s} {data[k].shape}")
