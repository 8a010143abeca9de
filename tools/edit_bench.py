"""Cost of region-constrained generation against the per-request joint call: d24 bf16 (incl. both decodes, the bench's sampling settings
cfg 4, top_k 900, top_p 0.96) eager at B = 512 and as one HIP graph at B = 8.  Three modes on one model in one process, interleaved call by
call so that clock and thermal drift fall on all alike:

    per_request   autoregressive_infer_cfg in per-request mode (uniform parameters) - the baseline, whose code the edit path does not touch
    edit_nothing  edit_infer_cfg with both sources given and all-False masks: every token free (the forced-token table is all -1)
    edit_square   control fully kept, the image kept outside a centred half-size square: 1177 of 1360 tokens forced

The forced-token table's launch, the host checks of masks and sources (one min/max read-back per source) and the copies of the masks are inside
the edit times.  Reports images/s of each, the spread of the baseline's repeats and the ratios to the baseline.

Expectation: edit_nothing at parity with the baseline, within the larger of 1 % and the spread of the baseline's own repeats (the rule of
tools/request_params_bench.py); the measured ratio is reported whether or not it meets that.

    python tools/edit_bench.py --out profiles/edit_d24.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG, TOP_K, TOP_P = 4.0, 900, 0.96
BASE, EDITS = 'per_request', ('edit_nothing', 'edit_square')


def lib_digest():
    try:
        return open(os.path.join(ROOT, 'controlvar_amd', 'csrc', 'build', 'digest.txt')).read().strip()[:16]
    except OSError:
        return None


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def compare(B, calls, reps, warmup):
    """calls: {mode: fn(i)} -> medians, the baseline's spread, the ratios and the verdict on edit_nothing"""
    modes = list(calls)
    times = {m: [] for m in modes}
    for i in range(warmup):
        for m in modes:
            timed(lambda: calls[m](i))
    for i in range(reps):
        for m in modes[i % len(modes):] + modes[:i % len(modes)]:           # rotate the order: no mode always runs behind the same one
            times[m].append(timed(lambda: calls[m](100 + i)))
    med = {m: statistics.median(v) for m, v in times.items()}
    res = {m: {'ms_median': round(med[m] * 1e3, 3), 'ms_all': [round(t * 1e3, 3) for t in times[m]], 'images_per_s': round(B / med[m], 2)} for m in modes}
    spread = (max(times[BASE]) - min(times[BASE])) / med[BASE]
    bound = max(0.01, spread)
    res.update(baseline_spread=round(spread, 5), bound=round(bound, 5))
    for m in EDITS:
        res[m + '_over_per_request'] = round(med[m] / med[BASE], 5)
    res['edit_nothing_within_bound'] = bool(med['edit_nothing'] / med[BASE] - 1.0 <= bound)
    return res


def requests(vae, B, dev):
    """sources (tokenised synthetic pictures, tiled to B) and the two mask sets, all on the device"""
    import torch
    from controlvar_amd.synth import synth_images
    n = min(B, 8)
    ctrl, img = (torch.cat(vae.img_to_idxBl(synth_images(n, 256, seed=s).to(dev)), dim=1).repeat((B + n - 1) // n, 1)[:B].contiguous() for s in (51, 52))
    nothing = torch.zeros(B, 16, 16, dtype=torch.bool, device=dev)
    square = torch.ones(B, 16, 16, dtype=torch.bool, device=dev)
    square[:, 4:12, 4:12] = False
    return {'edit_nothing': dict(src_ctrl=ctrl, keep_ctrl=nothing, src_img=img, keep_img=nothing),
            'edit_square': dict(src_ctrl=ctrl, keep_ctrl=True, src_img=img, keep_img=square)}


def run(a):
    import torch
    from controlvar_amd import models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, bf16, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; the per-request joint call '
                     '(uniform parameters) and edit_infer_cfg with nothing kept / with control kept and the image kept outside a centred 8 x 8 square of the '
                     '16 x 16 latent, interleaved call by call on one model, median of the timed calls of each',
           'acceptance': 'edit_nothing_over_per_request - 1 <= max(0.01, baseline_spread), baseline_spread = (max - min) / median of the per_request repeats',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    def uniform(B):
        return dict(cfg=[CFG] * B, top_k=[TOP_K] * B, top_p=[TOP_P] * B)

    # ---- eager, the headline batch
    B = a.eager_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    req = requests(vae, B, dev)
    calls = {BASE: lambda i: var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, **uniform(B))}
    for m in EDITS:
        calls[m] = lambda i, m=m: var.edit_infer_cfg(B, labels, types, g_seed=[i] * B, **req[m], **uniform(B))
    res = compare(B, calls, a.reps, a.warmup)
    out[f'eager_B{B}'] = res
    print(f'[edit_bench] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- captured, B = 8
    B = a.graph_batch
    labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
    req = requests(vae, B, dev)
    rows = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True)
    edit = var.graphed_edit_generator(B, source='ids', cfg=CFG, top_k=TOP_K, top_p=TOP_P)
    calls = {BASE: lambda i: rows(labels, types, g_seed=[i] * B)}
    for m in EDITS:
        calls[m] = lambda i, m=m: edit(labels, types, g_seed=[i] * B, **req[m])
    res = compare(B, calls, a.graph_reps, a.warmup + 1)
    calls['edit_square'](0)                                 # the table of the last replay is the square's, whichever mode was timed last
    res['forced_tokens_of_edit_square'] = int((edit.forced()[0] >= 0).sum())
    out[f'graph_B{B}'] = res
    print(f'[edit_bench] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=512)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=15, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 3 or a.graph_reps < 3:
        ap.error('at least three repeats per mode')
    out = run(a)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
