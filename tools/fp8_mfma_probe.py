"""How v_mfma_scale_f32_16x16x128_f8f6f4 sums its 128 e4m3 products: the probes behind DESIGN.md 4i and the bound of tests/fp8_ref.py, through
ops.gemm_fp8 with exact data (every operand an e4m3 value, every expected result an exact fp32 number; scales 1, no epilogue, fp32 output).

    window      one product 2^16 at k = 0 and 127 products 2^-j: how much of 127 * 2^-j arrives
    position    the same with the large product at k = 33 / 64 / 127
    group       the large product at k = 0, its seven neighbours k = 1..7 a factor 2^-d below it, the rest zero: the cut-off inside a group
    companion   the large product at k = 0 and ONE product 2^-12 below it at k = p: which positions share the large product's group
    ratios      |result - float64| in units of 2^-24 (1 + 2^-7) sum |q_a q_w| for random codes of one binade, four binades, all 127 magnitudes,
                K = 128 ... 6144, and for gaussian rows quantised by the row rule (the numpy restatement of it)

    python tools/fp8_mfma_probe.py [--out profiles/fp8_mfma_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

U = 2.0 ** -24 * (1 + 2.0 ** -7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import fp8_ref as F
    from controlvar_amd import ops
    dev = torch.device('cuda:0')

    def run(qa, sa, qw, sw):
        M, K = qa.shape
        N = qw.shape[0]
        c = torch.empty(M, N, device=dev)
        ops.gemm_fp8(torch.from_numpy(qa).to(dev), torch.from_numpy(sa).to(dev), torch.from_numpy(qw).to(dev), torch.from_numpy(sw).to(dev), c, M=M, N=N, K=K)
        torch.cuda.synchronize()
        return c.double().cpu().numpy()

    def exact(a, w):
        qa, qw = F.encode_rne(a), F.encode_rne(w)
        assert np.array_equal(F.decode(qa), a) and np.array_equal(F.decode(qw), w)          # the data is exact in e4m3
        got = run(qa, np.ones(16, np.float32), qw, np.ones(16, np.float32))
        assert (got == got[0, 0]).all()
        return float(got[0, 0])

    def ratio(qa, sa, qw, sw):
        got, ref = run(qa, sa, qw, sw), F.product_ref(qa, sa, qw, sw)
        S = (np.abs(F.decode(qa)) * sa.astype(np.float64)[:, None]) @ (np.abs(F.decode(qw)) * sw.astype(np.float64)[:, None]).T
        r = np.abs(got - ref) / (U * S)
        return {'worst': round(float(r.max()), 2), 'mean': round(float(r.mean()), 3)}

    out = {'device': torch.cuda.get_device_name(dev), 'unit_of_ratios': '2^-24 (1 + 2^-7) sum |q_a q_w|', 'window': [], 'position': [], 'group': [], 'companion': [],
           'ratios': []}
    big = 65536.0
    for j in range(0, 20, 2):                             # 2^-j = 2^-(j // 2) * 2^-(j - j // 2): both factors e4m3 values down to j = 18
        x, w = np.full((16, 128), 2.0 ** -(j // 2)), np.full((16, 128), 2.0 ** -(j - j // 2))
        x[:, 0] = w[:, 0] = 256.0
        out['window'].append({'small_product': f'2^-{j}', 'arrived': exact(x, w) - big, 'exact': 127 * 2.0 ** -j})
    for pos in (33, 64, 127):
        x, w = np.full((16, 128), 2.0 ** -4), np.full((16, 128), 2.0 ** -4)
        x[:, pos] = w[:, pos] = 256.0
        out['position'].append({'large_at_k': pos, 'arrived': exact(x, w) - big, 'exact': 127 * 2.0 ** -8})
    for d in range(6, 18):
        x, w = np.zeros((16, 128)), np.zeros((16, 128))
        x[:, :8], w[:, :8] = 2.0 ** (8 - d), 256.0
        x[:, 0] = 256.0
        out['group'].append({'neighbours_below_by': f'2^-{d}', 'arrived': exact(x, w) - big, 'exact': 7 * 2.0 ** (16 - d)})
    for pos in (1, 3, 7, 8, 15, 16, 31, 32, 64):
        x, w = np.zeros((16, 128)), np.zeros((16, 128))
        x[:, 0] = w[:, 0] = 256.0
        x[:, pos], w[:, pos] = 2.0 ** -4, 256.0
        out['companion'].append({'at_k': pos, 'arrived': exact(x, w) - big, 'exact': 16.0})
    rng = np.random.default_rng(0)
    one = np.ones(64, np.float32)
    for name, lo, hi in (('one binade [1, 2)', 0x38, 0x3F), ('four binades', 0x30, 0x4F), ('all 127 magnitudes', 0, 0x7E)):
        for K in (128, 384, 1536, 6144):
            def codes(shape):
                return (rng.integers(lo, hi + 1, size=shape).astype(np.uint8) | (rng.integers(0, 2, size=shape).astype(np.uint8) << 7)).astype(np.uint8)
            out['ratios'].append(dict(data=name, K=K, candidate=F.candidate_depth(K), **ratio(codes((64, K)), one, codes((64, K)), one)))
    for K in (1536, 6144):
        g = np.random.default_rng(K)
        qa, sa = F.quant_rows(g.standard_normal((256, K)).astype(np.float32))
        qw, sw = F.quant_rows((g.standard_normal((256, K)) * 0.02).astype(np.float32))
        out['ratios'].append(dict(data='gaussian rows quantised by the row rule', K=K, candidate=F.candidate_depth(K), **ratio(qa, sa, qw, sw)))
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
