"""Cost of regional guidance against the per-request joint call: d24 bf16 (incl. both decodes, the bench's sampling settings cfg 4, top_k 900,
top_p 0.96), eager at a batch whose K = 3 arena fits beside those of the other modes (B = 128: 512 transformer rows and a 102 GB K/V arena at K = 3;
the modes differ in rows per sample, so each keeps an arena of its own size in the allocator's cache) and as one HIP graph at B = 8.  Four modes on one model in one process, interleaved call by call so that clock and thermal drift fall on all alike:

    per_request   autoregressive_infer_cfg in per-request mode (uniform parameters): 2 rows per sample - the baseline
    region_k1     region_infer_cfg with one label and uniform maps: the same 2 rows, the weights read per token (bit for bit the baseline's images)
    region_k2     two labels, split left / right: 3 rows per sample
    region_k3     three labels in three vertical bands: 4 rows per sample

The weight table's launch, the host checks of the maps (finite, non-negative, no empty cell) and their upload are inside the region times.  Reports
images/s of each, the spread of the baseline's repeats, the ratios to the baseline beside the ratio of transformer rows, (K + 1) / 2, and the time
of the weight-table launch alone (HIP events around 20 launches).

Expectation: region_k1 at parity with the baseline, within the spread of the baseline's own repeats, (max - min) / median; the measured ratio is
reported whether or not it meets that.

--ab-tree DIR: a checkout of the parent commit with its library built, e.g.
    git worktree add /tmp/cvar_parent HEAD~1 && (cd /tmp/cvar_parent && python -m controlvar_amd.build)
The calls that existed before (tools/edit_bench.py: the per-request joint
call and edit_infer_cfg, which share the sampler's source file with the new kernels) are then timed from that tree and from this one in alternating
child processes, and the ratios this / parent are written beside the spread of the parent's own runs.  (The parent's library cannot be loaded into
this tree through CVAR_LIB: the binding refuses a library without the new entry points.)

    python tools/region_bench.py --out profiles/region_d24.json [--ab-tree /tmp/cvar_parent]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG, TOP_K, TOP_P = 4.0, 900, 0.96
BASE, REGIONS = 'per_request', ('region_k1', 'region_k2', 'region_k3')


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
    """calls: {mode: fn(i)} -> medians, the baseline's spread, the ratios and the verdict on region_k1"""
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
    bound = spread
    res.update(baseline_spread=round(spread, 5), bound=round(bound, 5))
    for k, m in enumerate(REGIONS, start=1):
        res[m + '_over_per_request'] = round(med[m] / med[BASE], 5)
        res[m + '_rows_over_per_request'] = (k + 1) / 2
    res['region_k1_within_bound'] = bool(med['region_k1'] / med[BASE] - 1.0 <= bound)
    return res


def bands(B, K, S, dev):
    """K vertical bands, one label each: (B, K, S, S) fp32 on the device"""
    import torch
    band = torch.clamp(torch.arange(S) * K // S, max=K - 1)
    return (band[None, None, None, :] == torch.arange(K)[None, :, None, None]).float().expand(B, K, S, S).contiguous().to(dev)


def table_time(var, B, K, dev, n=20):
    """ms per weight-table launch at this batch, from HIP events around n launches"""
    import torch
    S = var.cfg.pyramid.patch_nums[-1]
    reg, cf = bands(B, K, S, dev), torch.full((B, K), CFG, dtype=torch.float64, device=dev)
    out = var._region_table(B, K, reg, None, cf, True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        var._region_table(B, K, reg, None, cf, True, out)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n, 4)


def run(a):
    import torch
    from controlvar_amd import models
    dev = torch.device('cuda:0')
    bf = torch.bfloat16
    vae = models.build_vae(compute_dtype=bf).to(dev)
    var = models.build_control_var(vae, depth=a.depth, mask_type='interleave_append', multi_cond=True, compute_dtype=bf).to(dev).eval()
    S = var.cfg.pyramid.patch_nums[-1]
    out = {'config': f'd{a.depth} ControlVAR 256^2 incl. both decodes, bf16, cfg {CFG}, top_k {TOP_K}, top_p {TOP_P}, one GPU; the per-request joint call '
                     '(uniform parameters) and region_infer_cfg with K = 1 (uniform maps), 2 and 3 labels (vertical bands), interleaved call by call on one '
                     'model, median of the timed calls of each',
           'acceptance': 'region_k1_over_per_request - 1 <= baseline_spread, baseline_spread = (max - min) / median of the per_request repeats',
           'expectation': 'region_kK_over_per_request about (K + 1) / 2, the ratio of transformer rows: a supposition until measured here',
           'lib_digest': lib_digest(), 'device': torch.cuda.get_device_name(dev)}

    def uniform(B):
        return dict(top_k=[TOP_K] * B, top_p=[TOP_P] * B)

    def modes(B, joint, region):
        labels, types = torch.arange(B) % 1000, torch.arange(B) % 4
        maps = {K: bands(B, K, S, dev) for K in (1, 2, 3)}
        lab = {K: torch.stack([(labels + 37 * k) % 1000 for k in range(K)], dim=1) for K in (1, 2, 3)}
        calls = {BASE: lambda i: joint(labels, types, i)}
        for K, m in enumerate(REGIONS, start=1):
            calls[m] = lambda i, K=K: region[K](lab[K], types, maps[K], i)
        return calls

    # ---- eager
    B = a.eager_batch
    res = compare(B, modes(B, lambda labels, types, i: var.autoregressive_infer_cfg(B, labels, g_seed=[i] * B, cond_type=types, cfg=[CFG] * B, **uniform(B)),
                           {K: (lambda lab, types, maps, i: var.region_infer_cfg(B, lab, types, regions=maps, cfg=CFG, g_seed=[i] * B, **uniform(B)))
                            for K in (1, 2, 3)}), a.reps, a.warmup)
    res['table_launch_ms'] = {f'k{K}': table_time(var, B, K, dev) for K in (1, 2, 3)}
    out[f'eager_B{B}'] = res
    print(f'[region_bench] eager B={B}: ' + json.dumps(res), flush=True)

    # ---- captured, B = 8
    B = a.graph_batch
    rows = var.graphed_generator(B, cfg=CFG, top_k=TOP_K, top_p=TOP_P, per_request=True)
    graphs = {K: var.graphed_region_generator(B, K, top_k=TOP_K, top_p=TOP_P) for K in (1, 2, 3)}
    res = compare(B, modes(B, lambda labels, types, i: rows(labels, types, g_seed=[i] * B),
                           {K: (lambda lab, types, maps, i, K=K: graphs[K](lab, types, regions=maps, cfg=CFG, g_seed=[i] * B)) for K in (1, 2, 3)}),
                  a.graph_reps, a.warmup + 1)
    res['table_launch_ms'] = {f'k{K}': table_time(var, B, K, dev) for K in (1, 2, 3)}
    out[f'graph_B{B}'] = res
    print(f'[region_bench] graph B={B}: ' + json.dumps(res), flush=True)
    return out


def ab_existing(a):
    """tools/edit_bench.py (the per-request joint call and edit_infer_cfg: calls that existed before) from the parent's tree and from this one, in
    alternating child processes -> medians of each side, this / parent, and the spread of the parent's runs"""
    trees = {'parent': os.path.abspath(a.ab_tree), 'this': ROOT}
    runs = {k: [] for k in trees}
    for r in range(a.ab_rounds):
        for side in (('parent', 'this') if r % 2 == 0 else ('this', 'parent')):
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'edit.json')
                subprocess.run([sys.executable, os.path.join(trees[side], 'tools', 'edit_bench.py'), '--depth', str(a.depth), '--eager-batch', str(a.eager_batch),
                                '--graph-batch', str(a.graph_batch), '--reps', '3', '--graph-reps', '9', '--out', path], check=True, cwd=trees[side],
                               stdout=subprocess.DEVNULL, timeout=600)
                runs[side].append(json.load(open(path)))
                print(f'[region_bench] A/B round {r}, {side}: done', flush=True)
    out = {'what': 'tools/edit_bench.py from a checkout of the parent commit and from this tree, alternating child processes; ms medians of each run, '
                   'this / parent of the medians over the runs, and spread = (max - min) / median of the parent runs',
           'rounds': a.ab_rounds}
    for stage in (f'eager_B{a.eager_batch}', f'graph_B{a.graph_batch}'):
        for mode in ('per_request', 'edit_square'):
            ms = {side: [r[stage][mode]['ms_median'] for r in runs[side]] for side in trees}
            med = {side: statistics.median(v) for side, v in ms.items()}
            spread = (max(ms['parent']) - min(ms['parent'])) / med['parent']
            out[f'{stage}.{mode}'] = {'parent_ms': ms['parent'], 'this_ms': ms['this'], 'this_over_parent': round(med['this'] / med['parent'], 5),
                                      'parent_spread': round(spread, 5), 'within_parent_spread': bool(med['this'] / med['parent'] - 1.0 <= spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--eager-batch', type=int, default=128)
    ap.add_argument('--graph-batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5, help='timed eager calls per mode (at least 3)')
    ap.add_argument('--graph-reps', type=int, default=15, help='timed replays per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--ab-tree', default=None, help='a checkout of the parent commit with its library built: A/B of the calls that existed before')
    ap.add_argument('--ab-rounds', type=int, default=4, help='child-process runs per side')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 3 or a.graph_reps < 3:
        ap.error('at least three repeats per mode')
    ab = ab_existing(a) if a.ab_tree else None                # first: the children need the memory this process has not taken yet
    out = run(a)
    if ab is not None:
        out['existing_calls_against_parent'] = ab
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
