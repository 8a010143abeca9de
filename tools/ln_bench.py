#!/usr/bin/env python3
"""adaLN LayerNorm-modulate pass at the d24 shapes: time and effective HBM bandwidth (4 B read + 2 B written per element).
Then the wide kernels (include/cvar_wide.h) at C = 2304 / 2560 / CVAR_WIDE_CMAX beside the register-row kernel at C = 2048 - the yardstick - in the
three store forms (bf16, split [hi | lo | hi], e4m3), all four widths through the ops.*_wide wrappers (at C = 2048 they launch the kernel the old
entry points launch), and the HBM copy rate (a device-to-device copy of the same bytes) in the same process."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from controlvar_amd import _lib, ops
dev = torch.device('cuda:0')


def per_call_ms(f, reps=10):
    for _ in range(3): f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


C = 1536; R = 768; n_ada = 6 * C * 24 + 2 * C
ada = torch.randn(R, n_ada, device=dev) * 0.1
for l in (1, 16, 64, 169, 256):
    M = R * l
    x = torch.randn(M, C, device=dev)
    u = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
    ms = per_call_ms(lambda: ops.ln_modulate(x, ada, 2 * C, 4 * C, n_ada, l, u, M, C, 1e-6))
    print(f'rows {M:7d} (l={l:3d}): {ms * 1e3:8.1f} us  {6.0 * M * C / ms / 1e9:6.2f} TB/s', flush=True)
del ada, x, u

# ---- wide rows: R sequences of l rows (the modulation rows stay in cache, as in a pass of the model); bytes = 4 read + what the form writes
R, l = 64, 1024
M = R * l
base = {}
print(f'\nwide rows, M = {M} ({R} sequences x {l}): GB/s by store form (bytes: x read + the output written); ratio to C = 2048', flush=True)
for Cw in (2048, 2304, 2560, _lib.WIDE_CMAX):
    ada = torch.randn(R, 2 * Cw, device=dev) * 0.1
    x = torch.randn(M, Cw, device=dev)
    ldq = ops.fp8_ldq(Cw)
    outs = {'bf16': torch.empty(M, Cw, device=dev, dtype=torch.bfloat16), 'split3': torch.empty(M, 3 * Cw, device=dev, dtype=torch.bfloat16),
            'fp8': (torch.empty(M, ldq, device=dev, dtype=torch.uint8), torch.empty(M, device=dev))}
    calls = {'bf16': (lambda: ops.ln_modulate_wide(x, ada, 0, Cw, 2 * Cw, l, outs['bf16'], M, Cw, 1e-6), 6.0 * M * Cw),
             'split3': (lambda: ops.ln_modulate_split3_wide(x, ada, 0, Cw, 2 * Cw, l, outs['split3'], M, Cw, 1e-6), 10.0 * M * Cw),
             'fp8': (lambda: ops.ln_modulate_fp8_wide(x, ada, 0, Cw, 2 * Cw, l, *outs['fp8'], M, Cw, 1e-6, ldq=ldq), 4.0 * M * Cw + M * (ldq + 4.0))}
    src, dst = torch.empty(M * Cw * 3 // 4, device=dev), torch.empty(M * Cw * 3 // 4, device=dev)       # 3 M C bytes read + 3 M C written = the bf16 form's 6 M C
    line = f'C {Cw:5d}:'
    for form, (f, nbytes) in calls.items():
        gbs = nbytes / per_call_ms(f) / 1e6
        base.setdefault(form, gbs)
        line += f'  {form} {gbs:7.0f} GB/s ({gbs / base[form]:.2f})'
    line += f'  copy {6.0 * M * Cw / per_call_ms(lambda: dst.copy_(src)) / 1e6:7.0f} GB/s'
    print(line, flush=True)
    del ada, x, outs, src, dst
