#!/usr/bin/env python3
"""Recording of the sampler kernels for tests/test_gpu_sample_regression.py::test_sampler_kernels_bit_identical_to_the_previous_library.

Runs on the GPU against the library of the commit BEFORE cfg_sample_kernel and cfg_sample_rows_kernel were given one shared body (CVAR_LIB
points at that build) and writes sample_regression.npz: ids, kept-set sizes, margins, combined logits and soft embeddings of every launch
of test_gpu_sample_regression.sample_outputs.

    CVAR_LIB=/path/to/previous/libcvar_hip.so python tests/golden/make_sample_regression.py [output.npz]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

from test_gpu_sample_regression import sample_outputs

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'sample_regression.npz')
    np.savez_compressed(out, **sample_outputs(torch.device('cuda:0')))
    print(f'wrote {out}  {os.path.getsize(out) / 1024:.1f} KiB')
