"""Cost of sampler='torch' against the default counter sampler: d24 bf16 autoregressive_infer_cfg (incl. both decodes, the reference's
sampling defaults top_k=900, top_p=0.96, cfg 4) at B = 512 and B = 32, one model in one process, the two modes interleaved call by call
so that clock and thermal drift fall on both alike.  'torch' draws its Exp(1) noise with torch on a device generator (model.rng).

    python tools/sampler_modes_bench.py --out profiles/torch_sampler_d24.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def run(a):
    import torch
    from controlvar_amd import models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    var.rng = torch.Generator(device=dev)
    out = {'config': f'd{a.depth} ControlVAR autoregressive_infer_cfg 256^2 incl. both decodes, bf16, top_k 900, top_p 0.96, cfg 4, one GPU; '
                     f"'counter' and 'torch' (device generator) interleaved call by call on one model, median of {a.reps} calls each",
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}
    for B in a.batch:
        labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
        times = {'counter': [], 'torch': []}

        def call(mode, i):
            var.sampler = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            var.autoregressive_infer_cfg(B, labels, g_seed=i, cfg=4.0, top_k=900, top_p=0.96, cond_type=types)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for i in range(a.warmup):
            call('counter', i)
            call('torch', i)
        for i in range(a.reps):
            order = ('counter', 'torch') if i % 2 == 0 else ('torch', 'counter')
            for mode in order:
                times[mode].append(call(mode, 100 + i))
        res = {m: {'ms_median': round(statistics.median(v) * 1e3, 2), 'ms_min': round(min(v) * 1e3, 2), 'images_per_s': round(B / statistics.median(v), 2)}
               for m, v in times.items()}
        res['torch_over_counter'] = round(statistics.median(times['torch']) / statistics.median(times['counter']), 4)
        # the extra traffic: the Exp(1) noise is written by exponential_ and read by the sampler, one fp32 per code per token
        ntok = sum(var.cfg.pyramid.l)
        res['noise_bytes_per_generation'] = B * ntok * var.cfg.vocab * 4
        out[f'B{B}'] = res
        print(f'[sampler_modes] B={B}: ' + json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--batch', type=int, nargs='+', default=[512, 32])
    ap.add_argument('--reps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = run(a)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
