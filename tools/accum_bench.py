"""Cost of gradient accumulation on the d24 training step (bf16, B = 32 per micro-batch, one GPU), one process, the variants interleaved
round by round so that they see the same machine:

  (a) the plain step                        Trainer(), one step() = tokenizer + forward + backward + clip + AdamW + W^T refresh
  (b) a grad_accum = 4 window               Trainer(grad_accum=4): every call timed on its own (calls 1-3 skip the optimizer, call 4 runs it),
                                            and the window as a whole
  (c) forward_backward alone                the engine on pre-tokenized inputs, overwriting vs accumulating - the difference is what the
                                            accumulating stores (re-reading the gradient they add to) and the staging adds cost

    python tools/accum_bench.py --out profiles/accum_d24.json

Both trainers drive the same model, engine and optimizer (one set of activations in HBM); every timed region ends in a device synchronise."""
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


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2), 'n': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--accum', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1, help='untimed rounds')
    ap.add_argument('--out')
    a = ap.parse_args()
    import torch
    from controlvar_amd import models
    from controlvar_amd import train as T
    from controlvar_amd.synth import synth_images
    if not torch.cuda.is_available():
        raise SystemExit('accum_bench needs the GPU: nothing here can be timed without one')
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    B, N = a.batch, a.accum
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev)
    kw = dict(peak_lr=8e-5 * B / 512, weight_decay=0.08, sche='lin0', warmup_it=10, max_it=10000, clip=2.0, train_mode=True)
    plain = T.Trainer(var, vae, **kw)
    window = T.Trainer(var, vae, grad_accum=N, **kw)
    window.engine, window.opt = plain.engine, plain.opt                    # one engine: one set of activations and gradient buffers
    g = torch.Generator().manual_seed(0)
    batches = [(synth_images(B, 256, seed=10 + k).to(dev), synth_images(B, 256, seed=20 + k).to(dev), torch.randint(0, 1000, (B,), generator=g),
                torch.randint(0, 4, (B,), generator=g)) for k in range(N)]
    x, labels = plain.tokenize(batches[0][0], batches[0][1])
    eng = plain.engine

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_plain, t_micro, t_window, t_fb, t_fb_acc = [], [[] for _ in range(N)], [], [], []
    seed = 0
    for r in range(a.warmup + a.rounds):
        rec = r >= a.warmup
        im, mk, cls, ty = batches[0]
        seed += 1
        ms = timed(lambda: plain.step(im, mk, cls, ty, drop_seed=seed, mask_first=True))
        per = []
        for k in range(N):
            im, mk, cls, ty = batches[k]
            seed += 1
            per.append(timed(lambda: window.step(im, mk, cls, ty, drop_seed=seed, mask_first=True)))
        cls, ty = batches[0][2], batches[0][3]
        fb = timed(lambda: eng.forward_backward(cls, x, ty, labels, None, seed, True))
        fba = timed(lambda: eng.forward_backward(cls, x, ty, labels, None, seed, True, accumulate=True))
        if rec:
            t_plain.append(ms); t_window.append(sum(per)); t_fb.append(fb); t_fb_acc.append(fba)
            for k in range(N):
                t_micro[k].append(per[k])
    n_params = sum(p.numel() for p in var.parameters())
    grad_bytes = sum(b.numel() * 4 for b in eng.buckets)
    staging_bytes = sum(t.numel() * 4 for t in eng._staging.values())
    med = statistics.median
    out = {
        'config': f'd{a.depth} ControlVAR training step, bf16, B = {B} per micro-batch, frozen tokenizer inside the step, one GPU, one process, '
                  f'{a.rounds} interleaved rounds after {a.warmup} warm-up; host clock around a device synchronise',
        'lib_digest': lib_digest(),
        'parameters': n_params, 'gradient_buffer_GB': round(grad_bytes / 1e9, 3), 'staging_GB': round(staging_bytes / 1e9, 3),
        'a_plain_step': dict(summary(t_plain), samples_per_s=round(B / med(t_plain) * 1e3, 2)),
        'b_window': dict(summary(t_window), accum=N, samples_per_s=round(N * B / med(t_window) * 1e3, 2),
                         per_micro_batch=[summary(t) for t in t_micro],
                         note='calls 1..N-1: tokenizer + forward + backward; call N also clips, steps AdamW and refreshes W^T'),
        'c_forward_backward': {'overwrite': summary(t_fb), 'accumulate': summary(t_fb_acc),
                               'accumulate_minus_overwrite_ms': round(med(t_fb_acc) - med(t_fb), 2)},
        'mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
