"""Regional guidance in two calls on a depth-2 model with synthetic weights: two labels split left / right, then the same request with the border of
a source picture kept (edit_infer_cfg's masks).  Dumps both results as .npy, (B, 3, 512, 256) in [0, 1] - control on top, RGB below.  The weights are
synthetic, so the pictures show the plumbing, not a model's taste: nothing here judges image quality.

    python tools/region_demo.py [--out-dir region_demo] [--labels 207 980] [--cfg 4.0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out-dir', default='region_demo')
    ap.add_argument('--labels', type=int, nargs=2, default=[207, 980], help='the class on the left and the class on the right')
    ap.add_argument('--cfg', type=float, default=4.0)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from controlvar_amd import models
    from controlvar_amd.synth import synth_images
    dev = torch.device('cuda:0')
    vae = models.build_vae(ch=32, compute_dtype=torch.bfloat16).to(dev)
    var = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=torch.bfloat16).to(dev).eval()
    B, S = 2, var.cfg.pyramid.patch_nums[-1]
    labels = torch.tensor([a.labels] * B)
    types = torch.tensor([0, 1])
    left = (torch.arange(S) < S // 2).float()[None, None, None, :].expand(B, 1, S, S)
    regions = torch.cat([left, 1.0 - left], dim=1).contiguous()          # (B, 2, S, S): label 0 owns the left half, label 1 the right half
    request = dict(regions=regions, cfg=a.cfg, top_k=900, top_p=0.96, g_seed=[a.seed, a.seed + 1])
    split = var.region_infer_cfg(B, labels, types, **request)

    # the same request, the 3-cell border of a source picture kept in both halves
    ctrl, img = (vae.img_to_idxBl(synth_images(B, 16 * S, seed=s).to(dev)) for s in (51, 52))
    keep = torch.ones(B, S, S, dtype=torch.bool)
    keep[:, 3:S - 3, 3:S - 3] = False
    bordered = var.region_infer_cfg(B, labels, types, src_ctrl=ctrl, keep_ctrl=keep, src_img=img, keep_img=keep, **request)

    os.makedirs(a.out_dir, exist_ok=True)
    for name, x in (('split', split), ('split_kept_border', bordered)):
        path = os.path.join(a.out_dir, name + '.npy')
        np.save(path, x.float().cpu().numpy())
        print(f'[region_demo] {name}: {tuple(x.shape)} in [{float(x.min()):.3f}, {float(x.max()):.3f}] -> {path}')


if __name__ == '__main__':
    main()
