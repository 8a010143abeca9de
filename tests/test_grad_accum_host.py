"""Gradient accumulation, host side (no GPU): the entry points of include/cvar_accum.h and their ctypes table, the versions of the two older
headers, and the window bookkeeping that Trainer.step runs on (train.AccumWindow) - which call syncs, what `it` counts, the gradient scale."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['cvar_gemm_tn_acc', 'cvar_lora_wgrad_acc', 'cvar_wordembed_grad_acc', 'cvar_add_inplace']


@pytest.fixture(scope='module')
def lib():
    from controlvar_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.load()


def _declarations(header):
    """name -> list of parameter declarations, comments stripped"""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(cvar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        args = m.group(2).strip()
        out[m.group(1)] = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
    return out


def test_accum_entry_points_are_declared_exported_and_bound(lib):
    from controlvar_amd import _lib
    decl = _declarations('cvar_accum.h')
    assert sorted(decl) == sorted(NAMES) == sorted(_lib.ACCUM_SIGNATURES)
    assert not set(_lib.ACCUM_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SERVE_SIGNATURES))
    for name in NAMES:
        res, argtypes = _lib.ACCUM_SIGNATURES[name]
        assert hasattr(lib, name), f'{name} declared in include/cvar_accum.h but not exported'
        assert len(argtypes) == len(decl[name]), (name, len(argtypes), decl[name])
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res        # load() bound the third table


def test_accumulating_forms_are_their_namesakes_plus_one_flag():
    """each *_acc entry point = the cvar.h declaration of its namesake with `int accumulate` in front of the stream - in the header and in ctypes"""
    from controlvar_amd import _lib
    base, acc = _declarations('cvar.h'), _declarations('cvar_accum.h')
    for name in ('cvar_gemm_tn', 'cvar_lora_wgrad', 'cvar_wordembed_grad'):
        a, b = acc[name + '_acc'], base[name]
        norm = lambda d: re.sub(r'\s+', ' ', d)
        assert [norm(x) for x in a[:-2]] == [norm(x) for x in b[:-1]], name
        assert norm(a[-2]) == 'int accumulate' and norm(a[-1]) == norm(b[-1]) == 'void* stream'
        ta, tb = _lib.ACCUM_SIGNATURES[name + '_acc'][1], _lib.SIGNATURES[name][1]
        assert ta[:-2] == tb[:-1] and ta[-2] is _lib.c_i and ta[-1] is tb[-1] is _lib.c_p
    assert acc['cvar_add_inplace'] == ['float* y', 'const float* x', 'int64_t n', 'void* stream']


def test_the_older_headers_did_not_move(lib):
    from controlvar_amd import _lib
    assert _lib.ABI_VERSION == 22 and lib.cvar_abi_version() == 22
    assert _lib.SERVE_VERSION == 1 and lib.cvar_serve_version() == 1
    assert not set(NAMES) & set(_declarations('cvar.h')) and not set(NAMES) & set(_declarations('cvar_serve.h'))


def test_host_calls_refuse_bad_arguments_without_a_gpu(lib):
    """argument checks come before any launch: status CVAR_EINVAL (-1) for NULL pointers and empty sizes"""
    assert lib.cvar_add_inplace(None, None, 16, None) == -1
    assert lib.cvar_add_inplace(64, 128, 0, None) == -1
    assert lib.cvar_add_inplace(64, 130, 16, None) == -2                      # not 4-byte aligned: CVAR_EUNSUPPORTED
    assert lib.cvar_gemm_tn_acc(None, 128, None, 128, None, 128, 32, 128, 128, None, 0, None, 1, None) == -1
    assert lib.cvar_gemm_tn_acc(64, 128, 64, 128, 64, 128, 32, 100, 128, None, 0, None, 1, None) == -2      # Nn % 128
    assert lib.cvar_lora_wgrad_acc(None, 8, None, 16, 8, 8, 16, 1, 1.0, 0.0, 0, 0, None, 0, None, 16, 1, 1, None) == -1
    assert lib.cvar_wordembed_grad_acc(None, 64, 4, 0, None, 4, 1, 64, 32, None, None, None, 1, None) == -1


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize('bad', [0, -1, 1.5, None, '2', True])
def test_grad_accum_below_one_is_refused_in_words(bad):
    from controlvar_amd.train import AccumWindow, Trainer
    with pytest.raises(ValueError, match='grad_accum must be an integer >= 1'):
        AccumWindow(bad)
    with pytest.raises(ValueError, match='grad_accum must be an integer >= 1'):
        Trainer(None, None, peak_lr=1e-3, weight_decay=0.0, grad_accum=bad)          # refused before the model is touched


@pytest.mark.parametrize('n', [1, 2, 3, 5])
def test_window_bookkeeping(n):
    """call c (0-based) of a run is micro-batch c % n of window c // n: it overwrites iff it opens its window, syncs iff it closes it,
    and `it` - what the lr / wd schedule is evaluated at - counts closed windows"""
    from controlvar_amd.train import AccumWindow
    w = AccumWindow(n)
    for c in range(4 * n + 1):
        assert w.it == c // n
        micro, accumulate, sync = w.begin()
        assert w.begin() == (micro, accumulate, sync)                      # asking does not advance
        assert micro == c % n and accumulate == (c % n > 0) and sync == (c % n == n - 1)
        assert w.end() == sync
        assert w.it == (c + 1) // n
    w.it = 40                                                              # a resumed run sets the step count; the window position is its own
    assert w.begin()[0] == (4 * n + 1) % n and w.it == 40


def test_gradient_scale_is_the_mean_over_ranks_and_micro_batches():
    from controlvar_amd.train import AccumWindow
    assert AccumWindow.grad_scale(1, 1) == 1.0
    assert AccumWindow.grad_scale(8, 1) == 1.0 / 8                          # the plain data-parallel step: unchanged
    assert AccumWindow.grad_scale(2, 3) == 1.0 / 6
    assert AccumWindow.grad_scale(1, 4) == 0.25


def test_schedule_counts_optimizer_steps():
    """the lr Trainer.step applies is lr_wd_factors at `it`: the same for every micro-batch of a window, the next value only after the sync"""
    from controlvar_amd.train import AccumWindow, lr_wd_factors
    w = AccumWindow(3)
    seen = []
    for _ in range(9):
        seen.append(lr_wd_factors('lin0', 2e-3, 0.05, 0.05, w.it, 2, 50, wp0=0.005, wpe=0.01)[0])
        w.begin(); w.end()
    per_step = [lr_wd_factors('lin0', 2e-3, 0.05, 0.05, it, 2, 50, wp0=0.005, wpe=0.01)[0] for it in range(3)]
    assert seen == [per_step[0]] * 3 + [per_step[1]] * 3 + [per_step[2]] * 3
    assert per_step[0] < per_step[1] < per_step[2]                         # warm-up: the three values differ


def test_trainer_and_engine_signatures():
    import inspect
    from controlvar_amd import train as T
    assert inspect.signature(T.Trainer.__init__).parameters['grad_accum'].default == 1
    assert inspect.signature(T.TrainEngine.forward_backward).parameters['accumulate'].default is False
    assert inspect.signature(T.TrainEngine.backward).parameters['accumulate'].default is False
    assert inspect.signature(T.FusedAdamW.step).parameters['accum'].default == 1
