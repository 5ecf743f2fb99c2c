"""Parity at the sizes BASELINE.json's configs name (the launch plans, split-K slices, tiles and the eval fast path
that only exist at those sizes), against the CPU oracle on the same seeded inputs with identical explicit noise:
  C2  (2000, 1000) features, latent 32, B = 512: fp32 and bf16 compute (the benchmarked launch plan)
  C4  (2000, 1000, 500) features, latent 64, three modalities (generalised oracle; unpinned by the reference)
  C5  (5000, 2000) features, latent 64 (233 M parameters), fp32
  eval: embed / impute where the large-tile + fused eval-BatchNorm path runs (n >= 2048 rows, chunk boundaries,
        n > 65536 once) at rtol 1e-4 / atol 1e-5 (north_star) from identical weights.
Reference lines: jamie/jamie.py:611-741 (step), :806-837 (inference); jamie/model.py:116-282.
Run on the MI355X box:  pytest -m gpu"""
import numpy as np
import pytest
import torch

from oracle import jamie_oracle as orc
from test_hip_step import _noise_to_dev, assert_mostly_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def jam():
    import jamie_amd
    from jamie_amd import _native
    _native.require_gpu()
    return jamie_amd


def _synth(B, dims, seed=0, latent=16):
    """SURVEY.md §8(d) generator, standardised per feature."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((B, latent)).astype(np.float32)
    X = [torch.from_numpy(Z @ rng.standard_normal((latent, d)).astype(np.float32)
                          + .1 * rng.standard_normal((B, d)).astype(np.float32)) for d in dims]
    return [(x - x.mean(0)) / x.std(0) for x in X]


def _pair(jam, dims, L, B, mode, seed=666):
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    torch.manual_seed(seed)
    model = edModelVar(dims, L, pad_features=8 if (mode == 'bf16' and any(d % 8 for d in dims)) else 1)
    torch.manual_seed(seed)
    P, Bf = orc.init_state(dims, L)
    for v in P.values():
        v.requires_grad_(True)
    assert model.num_parameters() == orc.param_count(dims, L)
    eng = TrainEngine(model, B, compute_dtype=mode)
    return model, eng, P, Bf


def _grad(eng, model, ref):
    mine, sl = model.layout.reference_names()[ref]
    g = eng.grad_view(mine) if hasattr(eng, 'grad_view') else eng.g[mine]
    return (g if sl is None else g[sl]).cpu().numpy()


def _check_first_adam_step(eng, model, init_flat, lr=1e-3, norm=None):
    """clip_grad_norm_(1) + the FIRST Adam step restated on the engine's own gradient (jamie.py:739-741):
    coef = min(1, 1 / (||g|| + 1e-6)); m_hat = g c, v_hat = (g c)^2  ->  p = p0 - lr g c / (|g c| + 1e-8).
    Against the oracle's post-step weights only the bulk can agree: an element whose gradient is rounding noise
    (|g| <~ 1e-8: ~1 % of the BatchNorm shifts at these sizes, where gradients are O(1e-6)) moves by anything in
    [-lr, lr] in two correct fp32 implementations.  This check has no such freedom."""
    g = eng.grad_flat().double()
    if getattr(eng, '_g16_last', False) and not eng._direct_now:
        g = eng.grad16.double()           # bf16 weight-gradient buffer: the optimiser read EVERY range from it (rounded once)
    # (`norm`: the clip norm the engine itself used -- with bf16 weight gradients it is the norm of the fp32 accumulators, not
    #  of the rounded values the optimiser reads)
    coef = min(1.0, 1.0 / ((float(g.norm()) if norm is None else norm) + 1e-6))
    gc = g * coef
    want = init_flat.double() - lr * gc / (gc.abs() + 1e-8)
    err = (model.flat.double() - want).abs() - 1.2e-7 * want.abs()          # fp32 rounding of the stored parameter
    assert float(err.max()) < 2e-9 + 2e-6 * lr, float(err.max())


def _clone_state(P, Bf):
    P2 = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    return P2, {k: v.clone() for k, v in Bf.items()}


def _float64(P, Bf, X, noise):
    """The oracle's state, batch and noise in float64 (the same values).  A float64 step is a yardstick whose own rounding is
    far below the fp32 tolerances; an fp32 CPU step is not: at config 4 its decoders.0.0.weight gradient is 3.6e-3 (relative
    L2) from the float64 step when torch splits the reductions over 8 or 16 threads and 1e-6 on one thread."""
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    Bf64 = {k: v.double() if v.is_floating_point() else v.clone() for k, v in Bf.items()}
    n64 = {k: [[None if m is None else m.double() for m in v] if isinstance(v, list) else v.double() for v in vs]
           for k, vs in noise.items()}
    return P64, Bf64, [x.double() for x in X], n64


KINK_BAND = 1e-5       # fp32 rounding of a LeakyReLU input (BatchNorm output, O(1)): at most 4e-6 at config 4 (fp32 CPU step vs float64)


def _kink_rows(P, X, combined, noise, p):
    """Rows whose gradient is not defined to fp32 precision: a LeakyReLU input that the float64 step puts within KINK_BAND of the
    kink (and that dropout keeps) takes either branch in a correct fp32 implementation -- slope 1 or 0.01 for that element, i.e.
    a different gradient for its column's Linear row and bias and BatchNorm weight and bias.  (Config 4: one input at 2e-11 in
    decoders.0.1 moves decoders.0.0.weight by 3.6e-3 in relative L2 between the fp32 and the float64 step.)  From the
    pre-step float64 state `P`, the batch, the decoders' inputs `combined` and the noise: {parameter name: row indices}."""
    rows = {}
    for i in range(len(X)):
        for a, pre, masks in ((X[i], f'encoders.{i}', noise['enc_masks'][i]), (combined[i], f'decoders.{i}', noise['dec_masks'][i])):
            for (lin, bn), mask in zip(((0, 1), (4, 5)), masks):
                y = torch.nn.functional.batch_norm(orc.linear(P, f'{pre}.{lin}', a), None, None, P[f'{pre}.{bn}.weight'],
                                                   P[f'{pre}.{bn}.bias'], training=True, eps=orc.BN_EPS)
                near = (y.abs() < KINK_BAND) & ((mask > 0) if mask is not None else True)
                cols = sorted(set(near.nonzero()[:, 1].tolist()))
                if cols:
                    for name in (f'{pre}.{lin}.weight', f'{pre}.{lin}.bias', f'{pre}.{bn}.weight', f'{pre}.{bn}.bias'):
                        rows[name] = cols
                a = torch.nn.functional.leaky_relu(y, orc.LRELU_SLOPE)
                if mask is not None and p > 0:
                    a = a * (mask / (1 - p))
    return rows


def _drop_rows(t, rows):
    keep = np.ones(t.shape[0], dtype=bool)
    keep[rows] = False
    return t[keep]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _check_products_against_stored_operands(eng, model, noise, p):
    """LOCAL consistency of the bf16 step at full size, from the engine's own buffers after forward_backward: every
    GEMM launch's result equals the fp32-accumulated product of the bf16 operands the producing kernels stored (forward sums of
    the split-K slabs + bias; input gradients; all six weight gradients per modality, rounded once where the bf16 gradient
    buffer holds them), and every BatchNorm launch's bf16 output is the rounding of BN + LeakyReLU + dropout of the summed
    pre-activation it was given.  Tolerance 5e-5 in relative L2 (fp32 summation order only; measured 2e-5 .. 5e-5): a wrong
    scale, a dropped K slice or slab, or a mis-rounded operand is O(1e-2) or more.  The checker is torch on the GPU."""
    from jamie_amd.model import BN_EPS, LRELU_SLOPE
    bfl = lambda t: t.float()      # noqa: E731
    dn = _noise_to_dev(noise, p)
    for i in range(eng.M):
        w, wb, P_ = eng.ws[i], eng.wbf, model.p
        for a, lin, h in (('x', 'enc0', 'h1'), ('a1', 'enc1', 'h2'), ('e1', 'dec1', 'g2')):
            want = bfl(w[a + '_bf']) @ bfl(wb[f'm{i}.{lin}.W']).t() + P_[f'm{i}.{lin}.b']
            assert _rel(eng.rows(i, h)[0], want) < 5e-5, (i, lin, 'forward', _rel(eng.rows(i, h)[0], want))
        want_ml = bfl(w['a2_bf']) @ bfl(wb[f'm{i}.head.W']).t()
        assert _rel(w['ml'].sum(0), want_ml) < 5e-5, (i, 'head forward')
        if 'xh' in w:
            want = bfl(w['e2_bf']) @ bfl(wb[f'm{i}.dec2.W']).t() + P_[f'm{i}.dec2.b']
            assert _rel(w['xh'].sum(0), want) < 5e-5, (i, 'dec2 forward')
        # the two products inside the fused latent launches are exact fp32: decoder layer 0 forward, the heads' input gradient
        # (eng.rows: the BatchNorm launches' fp32 inputs are kept in panels of 16 columns; row-major copies for the checks)
        assert _rel(eng.rows(i, 'g1')[0], w['comb'] @ P_[f'm{i}.dec0.W'].t() + P_[f'm{i}.dec0.b']) < 1e-5, (i, 'dec0 forward (fp32)')
        assert _rel(eng.rows(i, 'da2')[0], w['dml'] @ P_[f'm{i}.head.W']) < 1e-5, (i, 'heads input gradient (fp32)')
        nd = w['sk']['d_comb']
        for dy, lin, out in (('dxhat', 'dec2', eng.rows(i, 'de2').sum(0)), ('de2', 'dec1', eng.rows(i, 'de1').sum(0)),
                             ('de1', 'dec0', w['dcomb'][:nd].sum(0)), ('da2', 'enc1', eng.rows(i, 'da1').sum(0))):
            want = bfl(w[dy + '_bf']) @ bfl(wb[f'm{i}.{lin}.W'])
            assert _rel(out, want) < 5e-5, (i, lin, 'input gradient', _rel(out, want))
        for dy, a, lin in (('dxhat', 'e2', 'dec2'), ('de2', 'e1', 'dec1'), ('de1', 'comb', 'dec0'), ('dml', 'a2', 'head'),
                           ('da2', 'a1', 'enc1'), ('da1', 'x', 'enc0')):
            k = f'm{i}.{lin}.W'
            want = bfl(w[dy + '_bf']).t() @ bfl(w[a + '_bf'])
            g16 = eng._g16_last and k[:-2] in eng.dw_partial
            got = bfl(eng.g16[k]) if g16 else eng.g[k]
            # (rounded to bf16 on both sides: an accumulator within ~1e-6 of a rounding boundary may land on the other side)
            assert _rel(got, want.to(torch.bfloat16).float() if g16 else want) < (2e-4 if g16 else 5e-5), (i, lin, 'weight gradient')
        # BatchNorm + LeakyReLU + dropout outputs from the summed pre-activations (slab 0 after the forward launch)
        for bn, h, a, kind, j in (('bn0', 'h1', 'a1', 'enc_masks', 0), ('bn1', 'h2', 'a2', 'enc_masks', 1),
                                  ('bn2', 'g1', 'e1', 'dec_masks', 0), ('bn3', 'g2', 'e2', 'dec_masks', 1)):
            hv = eng.rows(i, h)[0]
            mean, var = hv.mean(0), hv.var(0, unbiased=False)
            y = (hv - mean) * torch.rsqrt(var + BN_EPS) * P_[f'm{i}.{bn}.g'] + P_[f'm{i}.{bn}.b']
            y = torch.where(y > 0, y, LRELU_SLOPE * y)
            if p > 0:
                mk = dn[kind][i][j]
                y = y * torch.nn.functional.pad(mk, (0, y.shape[1] - mk.shape[1])).float() / (1 - p)
            got, want = w[a + '_bf'], y.to(torch.bfloat16)
            # (statistics summed in another order: a value within ~1e-7 of a rounding boundary may land on the other side)
            off = got != want
            assert float(off.float().mean()) < 2e-3 and _rel(bfl(got), bfl(want)) < 3e-4, (i, bn, float(off.float().mean()))
            np.testing.assert_allclose(w[bn + '.mean'].cpu().numpy(), mean.cpu().numpy(), rtol=1e-4, atol=1e-6)


# gradients of the decoder's first two layers and the BatchNorm between them: the reconstruction loss's gradient reaches them
# through BatchNorm backward passes that subtract its column mean and its projection on the normalised activation (dh = gamma
# invstd (dy - mean(dy) - xn mean(dy xn))): what is left is 6-13 x smaller than dy, so a relative difference in dy comes out
# 6-13 x larger (measured on both sides, profiles/r03_bf16_emulation_*.log: hip-vs-emulated 1.8e-3 -> 1.2e-2 and
# emulated-vs-fp32 3e-3 -> 3.9e-2 from decoders.i.8.weight to decoders.i.4.weight)
_AMPLIFIED = ('decoders.{}.0.weight', 'decoders.{}.1.weight', 'decoders.{}.1.bias', 'decoders.{}.4.weight')


def _bf16_step_vs_emulating_oracle(eng, model, P, Bf, X, corr, noise, p, anneal, init_flat):
    """The TIGHT parity check of the benchmarked arithmetic (bf16 GEMM operands, fp32 accumulation, bf16 weight
    gradients): the oracle restates the step with THE SAME roundings (`orc.train_step(emulate=, grad_bf16=)`: the operands of
    every product the engine reports as bf16 are rounded to nearest even where the HIP kernels store them; everything else
    fp32), so what is left between the two is fp32 summation order, a handful of LeakyReLU-kink / bf16-tie crossings, and
    nothing a wrong scale or a mis-rounded slab could hide behind.  Called after `eng.forward_backward` on the same batch
    and noise, BEFORE the optimiser step.  Losses 2e-3 (measured 3e-5); every gradient tensor 1e-2 in relative L2 (measured
    1e-5 .. 5e-3: bf16 rounding is chaotic -- two runs whose fp32 values differ by 1e-7 round a fraction of the operands to
    different neighbours, 4e-3 apart, and the noise settles at ~1e-3 per tensor whatever its origin), 3e-2 for the four
    tensors per modality behind an amplifying BatchNorm backward (`_AMPLIFIED`), the whole gradient 5e-3; the clip norm 1e-3;
    then the first Adam step exactly (restated on the engine's own gradient and norm) and its direction against the oracle's
    update.  What this end-to-end comparison cannot resolve below ~1e-3, `_check_products_against_stored_operands` does
    product by product at 5e-5."""
    if eng.fuse_bf16 and eng._fused_latent(None, None) and (corr is None or torch.equal(corr, torch.eye(corr.shape[0]))):
        _check_products_against_stored_operands(eng, model, noise, p)
    amplified = {t.format(i) for t in _AMPLIFIED for i in range(len(X))}
    prec, gbf = eng.operand_precision(None if corr is None or torch.equal(corr, torch.eye(corr.shape[0])) else corr)
    assert prec is not None and gbf == bool(eng.grad_bf16)
    init = {k: v.detach().clone() for k, v in P.items()}
    st = orc.train_step(P, Bf, orc.Adam(P.values(), 1e-3), X, corr, None, noise, p, anneal, return_grads=True,
                        emulate=prec, grad_bf16=gbf)
    ls = eng.read_losses()[0]
    np.testing.assert_allclose(ls, st['losses'], rtol=2e-3, atol=1e-6)
    for i in range(len(X)):
        assert_mostly_close(eng.ws[i]['mu'].cpu().numpy(), st['mus'][i].numpy(), rtol=0, atol=0, max_bad_frac=1.0,
                            rel_l2=2e-3, msg=f'mu{i}')
    worst, num, den = 0.0, 0.0, 0.0
    for ref in P:
        if orc.is_dead_bias(ref):
            continue
        want = st['grads'][ref]
        if gbf and want.dim() == 2:          # the large matrices live in the bf16 gradient buffer: rounded once
            want = orc.bf16_round(want)
        got = _grad(eng, model, ref)
        assert_mostly_close(got, want.numpy(), rtol=0, atol=0, max_bad_frac=1.0, rel_l2=3e-2 if ref in amplified else 1e-2,
                            msg=ref)
        worst = max(worst, float(np.linalg.norm(got - want.numpy()) / max(1e-30, np.linalg.norm(want.numpy()))))
        num += float(np.square(got.astype(np.float64) - want.numpy()).sum())
        den += float(np.square(want.double().numpy()).sum())
    assert (num / den) ** 0.5 < 5e-3, ('whole gradient', (num / den) ** 0.5)
    eng.optimizer_step()
    if eng.fused_norm:
        n_live = eng.n_dw_partials + eng.sq_ranges.blocks
        norm = float(torch.sqrt(eng.norm_partials[:n_live].double().sum()))
    else:
        norm = float(eng.grad_flat().double().norm())
    assert abs(norm - st['grad_norm']) < 1e-3 * st['grad_norm'], (norm, st['grad_norm'])
    _check_first_adam_step(eng, model, init_flat, norm=norm)
    sd = model.state_dict()
    for k, v in P.items():
        if orc.is_dead_bias(k) or v.dim() != 2:
            continue
        du, dr = sd[k].cpu() - init[k], v.detach() - init[k]
        # Adam's first step is lr * sign(g) wherever |g| >> 1e-8: the same direction as the oracle's except where a gradient
        # element is rounding noise around zero
        agree = float((torch.sign(du) == torch.sign(dr)).float().mean())
        assert agree > (0.985 if k in amplified else 0.995), (k, agree)     # (against the fp32 oracle: 0.93-0.97)
    return worst


# ------------------------------------------------------------------------------------------------------------
# C2 in the benchmarked dtype, at the benchmarked size
# ------------------------------------------------------------------------------------------------------------
def test_config2_bf16_full_size_step_vs_oracle(jam):
    """BASELINE config 2 as bench.py runs it: B = 512, (2000, 1000), latent 32, dropout 0.6, bf16 GEMM operands.  The launch
    plan at this size (256x128 / 128x128 large tiles, (3, 2) / (6, 3) K slices, grouped dW + dX launches with W and the
    activations read as stored, dW-epilogue gradient norm over 85 range chunks) exists at no smaller size.  One step vs the
    fp32 oracle within bf16 operand rounding: losses 2 %, gradients 10 % relative L2 (tolerances of the (520, 264) test);
    the fused norm is ||g||; post-step weights moved like the oracle's."""
    B, dims, L, p = 512, (2000, 1000), 32, 0.6
    model, eng, P, Bf = _pair(jam, dims, L, B, 'bf16')
    assert model.dropout == p and model.num_parameters() == 40345130
    assert eng.fused_norm and eng.gcfg['enc0'] in (23, 31) and eng.ws[0]['sk']['enc0'] > 1
    opt = orc.Adam(P.values(), 1e-3)
    X = _synth(B, dims)
    torch.manual_seed(42)
    noise = orc.draw_noise(dims, L, B, p)
    init = {k: v.detach().clone() for k, v in P.items()}
    P_e, Bf_e = _clone_state(P, Bf)
    init_flat = model.flat.clone()
    st = orc.train_step(P, Bf, opt, X, torch.eye(B), torch.zeros(B, B), noise, p, 0.5, return_grads=True)
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.5)
    eng.forward_backward(None, None, _noise_to_dev(noise, p))
    ls, total, _ = eng.read_losses()
    np.testing.assert_allclose(ls, st['losses'], rtol=2e-2, atol=1e-5)          # (how far bf16 operands are from fp32)
    for i in range(2):        # latents behind three bf16 products
        assert_mostly_close(eng.ws[i]['mu'].cpu().numpy(), st['mus'][i].numpy(), rtol=0, atol=0, max_bad_frac=1.0,
                            rel_l2=3e-2, msg=f'mu{i}')
    for ref in P:
        if orc.is_dead_bias(ref):
            continue
        assert_mostly_close(_grad(eng, model, ref), st['grads'][ref].numpy(), rtol=0, atol=0, max_bad_frac=1.0,
                            rel_l2=1e-1, msg=ref)
    want = float(eng.grad_flat().double().norm())
    # ... and the tight check: the oracle with the same operand roundings (optimiser step included)
    _bf16_step_vs_emulating_oracle(eng, model, P_e, Bf_e, X, torch.eye(B), noise, p, 0.5, init_flat)
    n_live = eng.n_dw_partials + eng.sq_ranges.blocks
    got = float(torch.sqrt(eng.norm_partials[:n_live].double().sum()))
    assert abs(got - want) < 5e-6 * want, (got, want)
    gnorm_ref = st['grad_norm']
    assert abs(got - gnorm_ref) < 5e-2 * gnorm_ref
    # Adam's first step moves every live element by ~lr * sign(g): compare the UPDATE with the oracle's
    sd = model.state_dict()
    for k in ('encoders.0.0.weight', 'encoders.1.4.weight', 'decoders.0.8.weight', 'fc_mus.1.weight', 'decoders.1.0.weight'):
        du = sd[k].cpu() - init[k]
        dr = P[k].detach() - init[k]
        agree = float((torch.sign(du) == torch.sign(dr)).float().mean())
        assert agree > 0.93, (k, agree)
        assert float(du.abs().max()) <= 1.001e-3
    assert torch.equal(eng.wbf['m0.enc0.W'].float(), model.p['m0.enc0.W'].to(torch.bfloat16).float())


@pytest.mark.parametrize('mode', ['bf16', 'f32'])
def test_config2_plan_replay_equals_eager_at_full_size(jam, mode):
    """The recorded launch plan at config 2's size replays bit-identically to eager stepping (device sampler, Philox
    noise): what bench.py times is the same arithmetic the step-vs-oracle tests check."""
    from jamie_amd import _native as nv
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    dims, L, B, N = (2000, 1000), 32, 512, 4096
    data = [x.cuda().contiguous() for x in _synth(N, dims, seed=3)]
    flats, losses = [], []
    for use_plan in (False, True):
        torch.manual_seed(9)
        model = edModelVar(dims, L)
        eng = TrainEngine(model, B, compute_dtype=mode, seed=21)
        eng.set_kl_anneal(0.5)
        idx = torch.zeros(B, dtype=torch.int32, device='cuda')
        if use_plan:
            plan = eng.make_plan(data, idx, N)
            for _ in range(3):
                eng.run_plan(plan)
        else:
            for _ in range(4):
                nv.sample_indices(idx, N, 0, False, eng.state, 200)
                eng.load_batch(data, [idx, idx])
                eng.step()
        flats.append(model.flat.clone())
        losses.append(eng.read_losses()[0])
    assert torch.equal(flats[0], flats[1])
    assert losses[0] == losses[1] and np.isfinite(losses[0]).all()


# ------------------------------------------------------------------------------------------------------------
# C1 at its own workload: 5k cells x (200, 100), latent 16, B = 512 > min(features) => sampling WITH replacement
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_config1_own_workload_step_vs_oracle(jam, mode):
    """BASELINE config 1 as the reference would run it: (200, 100) features, latent 16, B = 512.  `replace = min(features) <
    batch_size` (jamie.py:553, sic) is TRUE here, so the batch holds duplicate cells and the correspondence block
    `P[idx][:, idx]` row-normalised (jamie.py:586-589) is a general [B, B] matrix: the general latent kernels
    (`small_mm` on the exact-fp32 MFMA), not the fused identity path.  fp32: one step against the oracle (latents, losses,
    every gradient, post-step weights).  bf16 (100 features padded to 104): against the oracle with the same operand
    roundings -- here decoder layer 0 and the heads' input gradient are bf16 products too."""
    B, dims, L, N = 512, (200, 100), 16, 5000
    model, eng, P, Bf = _pair(jam, dims, L, B, mode, seed=13)
    p = model.dropout
    assert p == 0.6 and model.num_parameters() == 420166
    data = _synth(N, dims, seed=1)
    idx = np.random.default_rng(7).integers(0, N, B)                 # with replacement
    assert len(np.unique(idx)) < B
    corr = orc.p_block(None, idx, idx)
    assert not torch.equal(corr, torch.eye(B)) and float(corr.sum(1).min()) > 0.999
    X = [d[idx] for d in data]
    torch.manual_seed(5)
    noise = orc.draw_noise(dims, L, B, p)
    init_flat = model.flat.clone()
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.5)
    eng.forward_backward(corr.cuda().contiguous(), None, _noise_to_dev(noise, p))
    if mode == 'bf16':
        prec, _ = eng.operand_precision(corr)
        assert prec['dec0'][0] and prec['head'][1]                   # general correspondence: no fused fp32 products
        _bf16_step_vs_emulating_oracle(eng, model, P, Bf, X, corr, noise, p, 0.5, init_flat)
        return
    st = orc.train_step(P, Bf, orc.Adam(P.values(), 1e-3), X, corr, None, noise, p, 0.5, return_grads=True)
    for i in range(2):
        np.testing.assert_allclose(eng.ws[i]['z'].cpu().numpy(), st['zs'][i].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(eng.ws[i]['comb'].cpu().numpy(), st['combined'][i].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(eng.read_losses()[0], st['losses'], rtol=2e-4, atol=1e-6)
    for ref in P:
        if not orc.is_dead_bias(ref):
            assert_mostly_close(_grad(eng, model, ref), st['grads'][ref].numpy(), rtol=0, atol=0, max_bad_frac=1.0,
                                rel_l2=2e-3, msg=ref)
    eng.optimizer_step()
    _check_first_adam_step(eng, model, init_flat)
    sd = model.state_dict()
    for k, v in P.items():
        if not orc.is_dead_bias(k):
            assert_mostly_close(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-3, atol=2e-5, max_bad_frac=2e-2,
                                rel_l2=1e-2 if v.dim() == 1 else 5e-4, msg=k)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_config1_own_workload_plan_replay_equals_eager(jam, mode):
    """The recorded plan bench.py --config c1 replays (device sampler WITH replacement, correspondence block from the
    indices, general latent kernels) equals eager stepping bit for bit, and the drawn batches do contain duplicates."""
    from jamie_amd import _native as nv
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    dims, L, B, N = (200, 100), 16, 512, 5000
    flats, losses = [], []
    for use_plan in (False, True):
        torch.manual_seed(9)
        model = edModelVar(dims, L, pad_features=8 if mode == 'bf16' else 1)
        eng = TrainEngine(model, B, compute_dtype=mode, seed=21)
        data = eng.pad_cells([x.cuda().contiguous() for x in _synth(N, dims, seed=3)])
        eng.set_kl_anneal(0.5)
        idx = torch.zeros(B, dtype=torch.int32, device='cuda')
        if use_plan:
            plan = eng.make_plan(data, idx, N, replace=True)
            for _ in range(3):
                eng.run_plan(plan)
        else:
            for _ in range(4):
                nv.sample_indices(idx, N, 0, True, eng.state, 200)
                eng.load_batch(data, [idx, idx])
                nv.corr_from_indices(idx, idx, eng.corr)
                eng.step(eng.corr)
        assert len(torch.unique(idx)) < B and int(idx.min()) >= 0 and int(idx.max()) < N
        flats.append(model.flat.clone())
        losses.append(eng.read_losses()[0])
    assert torch.equal(flats[0], flats[1])
    assert losses[0] == losses[1] and np.isfinite(losses[0]).all()


# ------------------------------------------------------------------------------------------------------------
# C4: three modalities at (2000, 1000, 500), latent 64
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_config4_full_size_step_vs_generalised_oracle(jam, mode):
    """BASELINE config 4 at its per-step size: three fully paired modalities, (2000, 1000, 500) features, latent 64,
    B = 512, dropout 0.6.  The reference asserts two modalities (jamie.py:420), so the oracle is the build-defined
    generalisation (reduces to the reference for M = 2, tests/test_oracle_golden.py).  fp32: losses,
    every gradient tensor, the clip norm and the post-step weights.  bf16 (500 is not a multiple of 8: the engine pads
    the feature dimension internally): the bf16 tolerances.  The oracle's step runs in float64 (`_float64`); the few rows whose
    gradient rests on a LeakyReLU input within fp32 rounding of the kink are left out of the comparisons (`_kink_rows`)."""
    B, dims, L, p = 512, (2000, 1000, 500), 64, 0.6
    model, eng, P, Bf = _pair(jam, dims, L, B, mode, seed=31)
    assert model.num_parameters() == 42738887
    X = _synth(B, dims, seed=4)
    torch.manual_seed(77)
    noise = orc.draw_noise(dims, L, B, p)
    P_e, Bf_e = _clone_state(P, Bf)
    P, Bf, X64, noise64 = _float64(P, Bf, X, noise)
    P0 = {k: v.detach().clone() for k, v in P.items()}
    opt = orc.Adam(P.values(), 1e-3)
    st = orc.train_step(P, Bf, opt, X64, None, None, noise64, p, 0.6, return_grads=True)
    kink = _kink_rows(P0, X64, st['combined'], noise64, p)
    assert sum(len(r) for k, r in kink.items() if P0[k].dim() == 2) <= 64      # of 14 000 rows
    init_flat = model.flat.clone()
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.6)
    eng.forward_backward(None, None, _noise_to_dev(noise, p))
    ls, total, _ = eng.read_losses()
    bf = mode == 'bf16'
    np.testing.assert_allclose(ls, st['losses'], rtol=2e-2 if bf else 2e-4, atol=1e-5 if bf else 1e-6)
    for ref in P:
        if orc.is_dead_bias(ref):
            continue
        got, want = _grad(eng, model, ref), st['grads'][ref].numpy()
        if ref in kink:
            got, want = _drop_rows(got, kink[ref]), _drop_rows(want, kink[ref])
        assert_mostly_close(got, want, rtol=0, atol=0, max_bad_frac=1.0, rel_l2=1e-1 if bf else 2e-3, msg=ref)
    if bf:        # the tight check against the oracle with the same operand roundings (runs the optimiser step)
        _bf16_step_vs_emulating_oracle(eng, model, P_e, Bf_e, X, None, noise, p, 0.6, init_flat)
    else:
        eng.optimizer_step()
    gnorm = float(eng.grad_flat().double().norm())
    # 2e-3 like the gradients: an activation within rounding of the LeakyReLU kink takes the other branch in two correct fp32
    # implementations (profiles/r02_c5_grad_error_vs_fp64.log: the HIP step and the fp32 CPU oracle each differ from an
    # fp64 oracle by 1.5e-3 in a different set of tensors)
    assert abs(gnorm - st['grad_norm']) < (5e-2 if bf else 2e-3) * st['grad_norm']
    if not bf:
        _check_first_adam_step(eng, model, init_flat)
        sd = model.state_dict()
        for k, v in P.items():
            if not orc.is_dead_bias(k):
                got, want = sd[k].cpu().numpy(), v.detach().numpy()
                if k in kink:
                    got, want = _drop_rows(got, kink[k]), _drop_rows(want, kink[k])
                assert_mostly_close(got, want, rtol=1e-3, atol=2e-5, max_bad_frac=2e-2, rel_l2=1e-2 if v.dim() == 1 else 5e-4, msg=k)
        for k, v in Bf.items():
            if 'num_batches' not in k:
                np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_padded_feature_dimension_is_exact_and_stays_zero(jam, mode):
    """edModelVar(pad_features=8) at (100, 77) features (-> 104, 80): the initial weights, one fp32 step (losses, gradients,
    post-step weights: the tolerances of the unpadded tests) and eval-mode inference are those of the unpadded model =
    the oracle; after 20 more steps with Philox noise every padding element of the parameters, the Adam moments and the
    BatchNorm running means is still exactly zero; state_dict() has the reference's shapes."""
    from jamie_amd import _native as nv
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    B, dims, L, p = 128, (100, 77), 8, 0.6
    torch.manual_seed(5)
    model = edModelVar(dims, L, pad_features=8)
    torch.manual_seed(5)
    P, Bf = orc.init_state(dims, L)
    assert model.pdims == [104, 80] and model.num_parameters() == orc.param_count(dims, L)
    sd = model.state_dict()
    for k, v in P.items():
        assert torch.equal(sd[k].cpu(), v), k
        v.requires_grad_(True)
    eng = TrainEngine(model, B, compute_dtype=mode)
    opt = orc.Adam(P.values(), 1e-3)
    X = _synth(B, dims, seed=6, latent=6)
    torch.manual_seed(3)
    noise = orc.draw_noise(dims, L, B, p)
    st = orc.train_step(P, Bf, opt, X, torch.eye(B), torch.zeros(B, B), noise, p, 0.5, return_grads=True)
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.5)
    eng.forward_backward(None, None, _noise_to_dev(noise, p))
    bf = mode == 'bf16'
    np.testing.assert_allclose(eng.read_losses()[0], st['losses'], rtol=2e-2 if bf else 2e-4, atol=1e-5 if bf else 1e-6)
    for ref in P:
        if orc.is_dead_bias(ref):
            continue
        got, want = _grad(eng, model, ref), st['grads'][ref].numpy()
        assert got.shape == want.shape
        if bf:
            assert_mostly_close(got, want, rtol=0, atol=0, max_bad_frac=1.0, rel_l2=1.5e-1, msg=ref)    # small layers: less averaging
        else:
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-5 * max(1e-6, float(np.abs(want).max())) + 1e-8,
                                       err_msg=ref)
    eng.optimizer_step()
    if not bf:
        sd = model.state_dict()
        for k, v in P.items():
            if not orc.is_dead_bias(k):
                assert_mostly_close(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-3, atol=2e-5, max_bad_frac=1e-3,
                                    rel_l2=1e-3, msg=k)
        full = {k: v.detach() for k, v in P.items()}
        full.update(Bf)
        model.load_state_dict(full)
        model.eval()
        with torch.no_grad():
            np.testing.assert_allclose(model.embed(X[1], 1).cpu().numpy(), orc.transform_one(P, Bf, X[1], 1).numpy(),
                                       rtol=1e-4, atol=1e-5)
            imp = model.impute(X[1], [1, 0])
            assert imp.shape == (B, dims[0])
            np.testing.assert_allclose(imp.cpu().numpy(), orc.impute(P, Bf, X[1], 1, 0).numpy(), rtol=1e-4, atol=2e-5)
        model.train()
    # more steps on Philox noise through the device sampler: the padding never moves
    data = eng.pad_cells([x.cuda() for x in _synth(1024, dims, seed=7, latent=6)])
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    for _ in range(20):
        nv.sample_indices(idx, 1024, 0, False, eng.state, 200)
        eng.load_batch(data, [idx, idx])
        eng.step()
    assert np.isfinite(eng.read_losses()[1])
    lay = model.layout
    for buf in (model.flat, eng.exp_avg, eng.exp_avg_sq, eng.grad_flat()):
        views = lay.views(buf)
        for name, (off, shape) in lay.entries.items():
            r = lay.real[name]
            if r == shape:
                continue
            mask = torch.ones(shape, dtype=torch.bool, device='cuda')
            mask[tuple(slice(0, n) for n in r)] = False
            assert float(views[name][mask].abs().max()) == 0.0, name
    for name, v in model.bn.items():
        if name.endswith('.mean') and lay.real[name] != tuple(v.shape):
            assert float(v[lay.real[name][0]:].abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------------------------
# C5 dims: (5000, 2000), latent 64, fp32 (BASELINE config 5's per-GPU step)
# ------------------------------------------------------------------------------------------------------------
def test_config5_dims_step_vs_oracle(jam):
    """One fp32 step at config 5's dimensions (233 477 258 parameters; nothing above (2000, 1000) was compared before):
    losses, every gradient tensor in relative L2, the clip norm, post-step weights."""
    B, dims, L, p = 512, (5000, 2000), 64, 0.6
    model, eng, P, Bf = _pair(jam, dims, L, B, 'f32')
    assert model.num_parameters() == 233477258
    opt = orc.Adam(P.values(), 1e-3)
    X = _synth(B, dims, seed=5)
    torch.manual_seed(43)
    noise = orc.draw_noise(dims, L, B, p)
    st = orc.train_step(P, Bf, opt, X, torch.eye(B), torch.zeros(B, B), noise, p, 0.5, return_grads=True)
    init_flat = model.flat.clone()
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.5)
    eng.forward_backward(None, None, _noise_to_dev(noise, p))
    ls, total, _ = eng.read_losses()
    np.testing.assert_allclose(ls, st['losses'], rtol=2e-4, atol=1e-6)
    for ref in P:
        if orc.is_dead_bias(ref):
            continue
        assert_mostly_close(_grad(eng, model, ref), st['grads'][ref].numpy(), rtol=0, atol=0, max_bad_frac=1.0,
                            rel_l2=3e-3, msg=ref)
    eng.optimizer_step()
    # see the config-4 test for the 2e-3 (LeakyReLU kink crossings; profiles/r02_c5_grad_error_vs_fp64.log)
    assert abs(float(eng.grad_flat().double().norm()) - st['grad_norm']) < 2e-3 * st['grad_norm']
    _check_first_adam_step(eng, model, init_flat)
    # (which layers carry the kink-crossing noise depends on the summation order, i.e. on the split-K plan: 7e-4 on the gradients
    #  upstream of decoders.0.5 with the plan of rounds 1-2, 5e-4 upstream of encoders.0.5 with round 3's -- everywhere else 1e-6,
    #  tools/diag_c5_f32_plans.py, profiles/r03_diag_c5_f32_plans.log; Adam's first step is sign(g), so a first-layer matrix full of
    #  near-zero gradients turns that into 1.2e-3 on its weights)
    sd = model.state_dict()
    for k, v in P.items():
        if not orc.is_dead_bias(k):
            assert_mostly_close(sd[k].cpu().numpy(), v.detach().numpy(), rtol=1e-3, atol=2e-5, max_bad_frac=2e-2,
                                rel_l2=1e-2 if v.dim() == 1 else 2e-3, msg=k)


def test_config5_dims_bf16_step_vs_emulating_oracle(jam):
    """Config 5's dimensions in bf16 compute (DESIGN quotes its throughput): the losses of one step within 2 % of the
    fp32 oracle's (the distance of bf16 operands from fp32), then losses / every gradient tensor / clip norm / first Adam
    step against the oracle WITH THE SAME OPERAND ROUNDINGS, and the fused gradient norm equals ||g||."""
    B, dims, L, p = 512, (5000, 2000), 64, 0.6
    model, eng, P, Bf = _pair(jam, dims, L, B, 'bf16')
    X = _synth(B, dims, seed=5)
    torch.manual_seed(43)
    noise = orc.draw_noise(dims, L, B, p)
    P_e, Bf_e = _clone_state(P, Bf)
    with torch.no_grad():
        zs, comb, X_hat, mus, lv = orc.forward(P, Bf, X, torch.eye(B), train=True, p=p, noise=noise)
        want = [float(v) for v in orc.losses(X, zs, comb, X_hat, mus, lv, None, 0.5)]
    del P, Bf
    init_flat = model.flat.clone()
    eng.set_batch([x.cuda() for x in X])
    eng.set_kl_anneal(0.5)
    eng.forward_backward(None, None, _noise_to_dev(noise, p))
    ls = eng.read_losses()[0]
    np.testing.assert_allclose(ls, want, rtol=2e-2, atol=1e-5)
    gn = float(eng.grad_flat().double().norm())
    _bf16_step_vs_emulating_oracle(eng, model, P_e, Bf_e, X, torch.eye(B), noise, p, 0.5, init_flat)
    if eng.fused_norm:
        n_live = eng.n_dw_partials + eng.sq_ranges.blocks
        assert abs(float(torch.sqrt(eng.norm_partials[:n_live].double().sum())) - gn) < 5e-6 * gn


# ------------------------------------------------------------------------------------------------------------
# C5's ROW count: 1 000 000 cells x (5000, 2000) resident on one GPU (28 GB of fp32 + the raw copy): the 64-bit index paths
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def million_cells(jam):
    """Raw and device-standardised [1 000 000, 5000] / [1 000 000, 2000] fp32 matrices (56 GB of the 288 GB in all),
    generated on the GPU chunk by chunk; freed when the module's tests are done."""
    from jamie_amd import _native as nv
    N, dims = 1_000_000, (5000, 2000)
    gen = torch.Generator(device='cuda').manual_seed(17)
    raw, std, stats = [], [], []
    for d in dims:
        x = torch.empty(N, d, device='cuda', dtype=torch.float32)
        scale = 0.5 + torch.rand(d, device='cuda', generator=gen)
        shift = torch.randn(d, device='cuda', generator=gen)
        for r0 in range(0, N, 100_000):
            x[r0:r0 + 100_000].normal_(generator=gen).mul_(scale).add_(shift)
        out, mean, sd = nv.standardise_columns(x)
        raw.append(x); std.append(out); stats.append((mean, sd, scale, shift))
    torch.cuda.synchronize()
    yield N, dims, raw, std, stats
    del raw, std, stats
    torch.cuda.empty_cache()


def test_million_cells_device_standardise(jam, million_cells):
    """`jamie_col_stats` / `jamie_standardise` (preclass(axis=0), utilities.py:654-678) over 5e9 elements: element offsets pass
    2^31 at row 429 497 of the 5000-feature matrix and byte offsets pass 2^32 at row 214 749.  Statistics against torch in
    float64 on a set of columns, the standardised values against (x - mean) / std on rows on both sides of those marks."""
    N, dims, raw, std, stats = million_cells
    for i, d in enumerate(dims):
        mean, sd, scale, shift = stats[i]
        cols = torch.tensor([0, 1, d // 3, d - 2, d - 1], device='cuda')
        sub = raw[i][:, cols].double()
        np.testing.assert_allclose(mean[cols].cpu().numpy(), sub.mean(0).cpu().numpy(), rtol=0, atol=1e-9)
        np.testing.assert_allclose(sd[cols].cpu().numpy(), sub.std(0, unbiased=False).cpu().numpy(), rtol=1e-9)
        assert float((mean.float() - shift).abs().max()) < 0.02 and float((sd.float() / scale - 1).abs().max()) < 0.01
        rows = torch.tensor([0, 214_748, 214_749, 429_496, 429_497, 429_498, 858_993, N - 2, N - 1], device='cuda')
        want = ((raw[i][rows].double() - mean) / sd).float()
        assert torch.equal(std[i][rows], want) or float((std[i][rows] - want).abs().max()) < 1e-6
        # a full pass: every standardised column has mean 0 and population std 1
        m = std[i].mean(0, dtype=torch.float64)
        assert float(m.abs().max()) < 1e-5
        q = torch.zeros(d, device='cuda', dtype=torch.float64)
        for r0 in range(0, N, 100_000):
            q += std[i][r0:r0 + 100_000].double().square().sum(0)
        assert float((q / N - 1).abs().max()) < 1e-4


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_million_cells_sampler_gather_and_steps(jam, million_cells, mode):
    """BASELINE config 5's row count on one GPU: the device sampler draws B = 512 DISTINCT rows of 1 000 000 without
    replacement (jamie.py:553-556: min(features) = 2000 >= 512), the gather (fp32 rows; bf16 mode: + the bf16 copy) returns
    exactly `data[idx]` -- also for hand-picked rows beyond element offset 2^31 and byte offset 2^32 and the last row --, and three
    recorded-plan steps at (5000, 2000), latent 64 stay finite and keep drawing from the whole range."""
    from jamie_amd import _native as nv
    from jamie_amd.engine import TrainEngine
    from jamie_amd.model import edModelVar
    N, dims, raw, std, stats = million_cells
    B, L = 512, 64
    torch.manual_seed(3)
    model = edModelVar(dims, L)
    eng = TrainEngine(model, B, compute_dtype=mode, seed=5)
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    picked = torch.tensor([0, 214_748, 214_749, 429_496, 429_497, 429_498, 536_871, 858_993, 999_998, N - 1], dtype=torch.int32)
    idx[:picked.numel()] = picked.cuda()
    idx[picked.numel():] = torch.arange(600_000, 600_000 + B - picked.numel(), dtype=torch.int32, device='cuda') * 1
    eng.load_batch(std, [idx, idx])
    for i in range(2):
        assert torch.equal(eng.ws[i]['x'], std[i][idx.long()])
        if mode == 'bf16':
            assert torch.equal(eng.ws[i]['x_bf'], std[i][idx.long()].to(torch.bfloat16))
    seen_hi = 0
    for _ in range(3):
        nv.sample_indices(idx, N, 0, False, eng.state, 200)
        eng.load_batch(std, [idx, idx])
        assert len(torch.unique(idx)) == B and int(idx.min()) >= 0 and int(idx.max()) < N
        seen_hi += int((idx > 429_497).sum())
        for i in range(2):
            assert torch.equal(eng.ws[i]['x'], std[i][idx.long()])
        eng.step()
    assert seen_hi > 3 * B // 4                                   # (57 % of the rows lie beyond 2^31 elements)
    plan = eng.make_plan(std, idx, N)
    for _ in range(3):
        eng.run_plan(plan)
    ls, total, _ = eng.read_losses()
    assert np.isfinite(ls).all() and np.isfinite(total)
    assert len(torch.unique(idx)) == B and int(idx.max()) < N and int(idx.max()) > 429_497
    if eng._plan_keep[1] is not None:      # the plan's gather rode in clip + Adam: the batch in the workspace is the NEXT one
        for i in range(2):
            assert torch.equal(eng.ws[i]['x'], std[i][idx.long()])
    del eng, model, plan
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------
# eval fast path: many rows
# ------------------------------------------------------------------------------------------------------------
def _seeded_eval_model(jam, dims, L, seed=11):
    """Random weights with NON-trivial BatchNorm affine parameters and running statistics (a fresh model has gamma = 1,
    beta = 0, mean = 0, var = 1, which would not exercise the fused eval-BN epilogue)."""
    from jamie_amd.model import edModelVar
    torch.manual_seed(seed)
    P, Bf = orc.init_state(dims, L)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in P.items():
        parts = k.split('.')
        is_bn = parts[0] in ('encoders', 'decoders') and parts[2] in ('1', '5')
        if is_bn and k.endswith('.weight'):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif is_bn and k.endswith('.bias'):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
    for k, v in Bf.items():
        if k.endswith('running_mean'):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith('running_var'):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
    model = edModelVar(dims, L)
    full = dict(P)
    full.update(Bf)
    model.load_state_dict(full)
    model.eval()
    return model, P, Bf


@pytest.mark.parametrize('x3', [True, False])
def test_eval_fast_path_many_rows_vs_oracle(jam, x3):
    """embed / impute at (2000, 1000) where the large tile + fused eval-BatchNorm epilogue run (n >= 2048 rows) -- on the bf16
    matrix pipe (configuration 21: three-piece cuts of every fp32 element, the default) and on the fp32 pipe (configuration 17):
    n = 5000 (not a tile multiple), chunked so that a chunk boundary and a short (< 2048 rows: default tile) last chunk
    are both crossed; rtol 1e-4 / atol 1e-5 against the oracle from identical weights (north_star's inference claim)."""
    dims, L = (2000, 1000), 32
    model, P, Bf = _seeded_eval_model(jam, dims, L)
    type(model).EVAL_X3 = x3
    try:
        _eval_fast_path(model, P, Bf, dims, 21 if x3 else 17)
    finally:
        type(model).EVAL_X3 = True


def _eval_fast_path(model, P, Bf, dims, cfg):
    assert model._eval_cfg(4096, 2000, 2000) == cfg
    assert model._eval_cfg(1000, 2000, 2000) == -1
    n = 5000
    X = _synth(n, dims, seed=8)
    with torch.no_grad():
        ref_e = [orc.transform_one(P, Bf, X[i], i).numpy() for i in range(2)]
        ref_i = [orc.impute(P, Bf, X[i], i, 1 - i).numpy() for i in range(2)]
    for i in range(2):
        for chunk in (65536, 2560):
            np.testing.assert_allclose(model.embed(X[i], i, chunk=chunk).cpu().numpy(), ref_e[i], rtol=1e-4, atol=1e-5,
                                       err_msg=f'embed {i} chunk {chunk}')
            np.testing.assert_allclose(model.impute(X[i], [i, 1 - i], chunk=chunk).cpu().numpy(), ref_i[i], rtol=1e-4,
                                       atol=1e-5, err_msg=f'impute {i} chunk {chunk}')
        # the chunked result is the unchunked one, bit for bit (rows are independent in eval mode)
        assert torch.equal(model.embed(X[i], i, chunk=2560), model.embed(X[i], i, chunk=65536))


def test_eval_more_rows_than_one_chunk_vs_oracle(jam):
    """n = 70 001 > 65 536 rows (the default chunk) of the 1000-feature modality: embeddings and imputed (2000-feature)
    rows of the default chunking against the oracle; checked on the rows around the chunk boundary and a random sample
    (the whole imputed matrix would be 560 MB of comparison)."""
    dims, L = (2000, 1000), 32
    model, P, Bf = _seeded_eval_model(jam, dims, L, seed=12)
    n = 70001
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((n, dims[1])).astype(np.float32))
    emb = model.embed(x, 1).cpu().numpy()
    assert emb.shape == (n, L)
    with torch.no_grad():
        ref = orc.transform_one(P, Bf, x, 1).numpy()
    np.testing.assert_allclose(emb, ref, rtol=1e-4, atol=1e-5)
    rows = np.unique(np.concatenate([np.arange(65530, 65545), [0, n - 1], rng.integers(0, n, 2000)]))
    imp = model.impute(x, [1, 0])
    assert imp.shape == (n, dims[0])
    with torch.no_grad():
        ref_i = orc.impute(P, Bf, x[rows], 1, 0).numpy()
    np.testing.assert_allclose(imp[torch.from_numpy(rows).cuda()].cpu().numpy(), ref_i, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------
# the loop users call, against the reference's fixtures
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['g3_multistep', 'g4_replace', 'g5_F_pfratio', 'g6_zeros', 'g7_cosine', 'g8_klquirk',
                                  'g9_earlystop', 'g10_midsize'])
def test_facade_loop_replays_reference_fixture(jam, name):
    """`JAMIE.fit_transform` itself (not the engine driven by the test) under `np.random.seed(meta.np_seed)` with the
    fixture's dropout masks / eps fed through the facade's noise seam, against the reference run that produced the fixture
    (jamie/jamie.py:546-583 sampler, :630-632 KL anneal per epoch, :729-731 best batch loss, :751-761 loss history,
    :777-792 early stop, :794-804 output):
      * the sampler's index stream equals the reference's `np.random.choice` stream bit for bit ('diag' with and without
        replacement, 'zeros' with unequal row counts);
      * `loss_history` has the reference's number of epochs — g9 STOPS EARLY (12 of 60 epochs; its streak decisions have
        margins >= 0.12 against min_increment = 0.25) — and its values (tolerances of the engine-level replay);
      * the returned embeddings in relative L2 (eval-mode outputs after training depend on Adam-amplified rounding noise
        in the dead biases in the reference as much as here, tests/test_hip_step.py)."""
    import contextlib
    import io
    from golden_util import Golden
    g = Golden(name)
    m = g.meta
    c = dict(m['ctor'])
    data = [g['data0'].astype(np.float64), g['data1'].astype(np.float64)]
    kw = dict(output_dim=m['L'], batch_size=m['B'], epoch_DNN=m['epochs'], pca_dim=None, use_f_tilde=m['has_F'],
              log_DNN=10 ** 9, manual_seed=666, sampler='numpy')
    if m['has_F']:
        kw['match_result'] = [g['F']]
    kw.update(c)
    jm = jam.JAMIE(**kw)
    jm._noise_source = lambda s: _noise_to_dev(g.noise(s), m['p'])
    calls = []
    orig = np.random.choice

    def choice(*a, **k):
        r = orig(*a, **k)
        calls.append(np.asarray(r).copy())
        return r
    np.random.seed(m['np_seed'])
    np.random.choice = choice
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            emb = jm.fit_transform(dataset=[d.copy() for d in data], P=g['P'] if m['has_P'] else None)
    finally:
        np.random.choice = orig
    assert jm.sampling_method == m['sampling_method'] and jm.model.dropout == m['p']
    ch = g['choice']
    assert len(calls) == len(ch), (len(calls), len(ch))
    for a, b in zip(calls, ch):
        assert np.array_equal(a, b)
    want = g['loss_history']
    got = np.array([jm.loss_history[k] for k in m['loss_names']])
    assert got.shape == want.shape, (got.shape, want.shape)        # same number of epochs: same stopping decision
    if name == 'g9_earlystop':
        assert want.shape[1] == 12 < m['epochs']
    big_lr = c.get('model_lr', 1e-3) > 1e-2
    np.testing.assert_allclose(got, want, rtol=5e-2 if big_lr else 2e-3, atol=1e-5)
    for i in range(2):
        assert emb[i].shape == g[f'emb{i}'].shape and emb[i].dtype == np.float32
        assert_mostly_close(emb[i], g[f'emb{i}'], rtol=0, atol=0, max_bad_frac=1.0, rel_l2=0.1 if big_lr else 1.5e-2,
                            msg=f'emb{i}')
