"""512 x 512 generation rate of a d16 ControlVAR beside its 256 x 256 rate, and the cost of the S = 32 quantizer calls.

One process, one GPU, bf16, autoregressive_infer_cfg incl. both decodes with the reference's sampling defaults (cfg 4, top_k 900, top_p 0.96):
per batch size the 512 x 512 model (PATCH_NUMS_512, 4 480 joint tokens) and the 256 x 256 model (680 x 2 tokens) of the same depth, warm-up plus
`--reps` timed calls each, median / min / max, and the bytes of the K/V arena the model allocated.  A batch that does not fit is replaced by the
largest smaller one that does.  Then `cvar_ms_next_input` (every scale of a generation, 2 B maps) and `cvar_ms_encode` (B maps) at S = 32 on
preallocated buffers: HIP events around `--inner` back-to-back calls, divided by their number, so the figure is the kernel's time unless a call is
shorter than a host launch.  Nothing is asserted: there is no earlier number at this resolution; the file is the record.

    python tools/res512_bench.py --out profiles/res512_d16.json
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


def stats_ms(v):
    return {'ms_median': round(statistics.median(v), 4), 'ms_min': round(min(v), 4), 'ms_max': round(max(v), 4), 'n': len(v)}


def event_ms(torch, fn, reps, inner, warmup=2):
    """per-call ms of `inner` back-to-back calls between one pair of events, `reps` times"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def generation(torch, var, B, a):
    """warm-up + timed generations at batch B; None when the batch does not fit"""
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4

    def call(i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        var.autoregressive_infer_cfg(B, labels, g_seed=i, cfg=4.0, top_k=900, top_p=0.96, cond_type=types)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    try:
        for i in range(a.warmup):
            call(i)
        ms = [call(100 + i) for i in range(a.reps)]
        py = var.cfg.pyramid
        res = stats_ms(ms)
        res['B'] = B
        res['images_per_s'] = round(B / statistics.median(ms) * 1e3, 3)
        res['tokens_per_image'] = py.L
        res['us_per_token'] = round(statistics.median(ms) * 1e3 / (B * py.L), 3)
        res['kv_arena_bytes'] = sum(t.numel() * t.element_size() for _, t in (var._arena or {}).values())     # as allocated: CFG doubles the rows
    except torch.cuda.OutOfMemoryError:
        res = None
    var._arena = None
    torch.cuda.empty_cache()
    return res


def run(a):
    import torch
    from controlvar_amd import models, ops
    from controlvar_amd.spec import DEFAULT_PATCH_NUMS, PATCH_NUMS_512
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    out = {'config': f'd{a.depth} ControlVAR autoregressive_infer_cfg incl. both decodes (ch 160 VQVAE), bf16, cfg 4, top_k 900, top_p 0.96, one GPU; '
                     f'{a.warmup} warm-up + {a.reps} timed calls per entry, wall clock around a synchronised call; quantizer entry points on '
                     f'preallocated buffers, HIP events around {a.inner} back-to-back calls, ms per call',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev), 'generation': {}, 'quantizer_S32': {}}
    built = {}
    for tag, pns in (('512', PATCH_NUMS_512), ('256', DEFAULT_PATCH_NUMS)):
        vae = models.build_vae(compute_dtype=bf, v_patch_nums=pns).to(dev)
        var = models.build_control_var(vae, depth=a.depth, patch_nums=pns, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
        built[tag] = (vae, var)
    for B in a.batch:
        entry = {}
        for tag, (vae, var) in built.items():
            b, res = B, generation(torch, var, B, a)
            while res is None and b > 1:                             # does not fit: step down by B / 8 to the largest batch that does
                b = max(1, b - max(1, B // 8))
                res = generation(torch, var, b, a)
            if res is None:
                res = {'error': 'out of memory'}
            elif b != B:
                res['requested_B'] = B
            entry[tag] = res
        if 'ms_median' in entry['512'] and 'ms_median' in entry['256']:
            entry['us_per_token_512_over_256'] = round(entry['512']['us_per_token'] / entry['256']['us_per_token'], 3)
        out['generation'][f'B{B}'] = entry
        print(f'[res512] B={B}: ' + json.dumps(entry), flush=True)
    # ---- the two C entry points at S = 32
    vae = built['512'][0]
    P = vae._pack()
    pns = list(PATCH_NUMS_512)
    for B in a.qbatch:
        f_hat = torch.zeros(B, 2, 32, 32, 32, device=dev)
        per_scale = []
        for si, pn in enumerate(pns):
            last = si + 1 == len(pns)
            pnn = pn if last else pns[si + 1]
            idx = torch.randint(0, 4096, (B, 2 * pn * pn), device=dev, dtype=torch.int32)
            tok = None if last else torch.empty(B, 2 * pnn * pnn, 32, device=dev)        # as in a generation: no tokens after the last scale
            down_off = 0 if last else P['tab_off'][si + 1]
            per_scale.append(statistics.median(event_ms(torch, lambda: ops.ms_next_input(
                idx, P['E'], P['phi_w'], P['phi_b'], P['up'], P['down'], f_hat, tok, B, 2, pn, pnn, 32, 32, P['phi_map'][si], P['tab_off'][si], down_off),
                a.reps, a.inner)))
        f = torch.randn(B, 32, 32, 32, device=dev)
        ids = torch.empty(B, sum(p * p for p in pns), device=dev, dtype=torch.int32)
        enc = event_ms(torch, lambda: ops.ms_encode(f, P['E'], vae.V, P['phi_w'], P['phi_b'], P['phi_map'], pns, P['up'], P['down'], ids, None, None,
                                                    B, 32, 32), a.reps, a.inner)
        q = {'next_input_ms_per_scale': [round(x, 4) for x in per_scale], 'next_input_ms_per_generation': round(sum(per_scale), 4),
             'ms_encode': stats_ms(enc)}
        gen = out['generation'].get(f'B{B}', {}).get('512', {})
        if gen.get('B') == B:
            q['next_input_share_of_generation'] = round(sum(per_scale) / gen['ms_median'], 5)
        out['quantizer_S32'][f'B{B}'] = q
        print(f'[res512] quantizer B={B}: ' + json.dumps(q), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=16)
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--qbatch', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--inner', type=int, default=10, help='back-to-back quantizer calls between one pair of events')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = run(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
