#!/usr/bin/env python3
"""Recording of the S = 16 quantizer kernels for tests/test_gpu_res512.py::test_s16_kernels_bit_identical_to_the_previous_library.

Runs on the GPU against the library of the commit BEFORE the S = 32 kernels were added (CVAR_LIB points at that build) and writes
msq16_regression.npz: ids, f_hat, margins and next-input outputs of two seeded feature batches (test_gpu_res512.msq16_outputs).

    CVAR_LIB=/path/to/previous/libcvar_hip.so python tests/golden/make_msq16_regression.py [output.npz]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

from test_gpu_res512 import msq16_outputs

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'msq16_regression.npz')
    np.savez_compressed(out, **msq16_outputs(torch.device('cuda:0')))
    print(f'wrote {out}  {os.path.getsize(out) / 1024:.1f} KiB')
