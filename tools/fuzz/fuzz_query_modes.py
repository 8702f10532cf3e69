#!/usr/bin/env python3
"""Fuzz campaign of the four single-launch query modes (MODE_CENTROIDAL, MODE_FRAMES, MODE_CORIOLIS, MODE_FD_CRB) in the
HOST EMULATION of the kernel core (tests/query_emul.py: the kernel sources compiled for the CPU) against their
restatements (tests/centroidal_ref.py, frames_ref.py, coriolis_ref.py, fd_crb_ref.py), on random trees of up to 64 links
(tests/query_modes_ref.py draw_tree: chains of 1 .. 64 links, serial to bushy, fixed / floating base, general / planar /
aligned axes; every tenth a hub with 7 .. 12 legs).  Every campaign starts with the three fixed trees of
query_modes_ref.FIXED_TREES: 64 links in one serial chain, 33 links (the smallest tree that takes a whole wave per
environment) and twelve legs of five links on one hub.  fp64 and fp32, N = 3; the outputs start as NaN and every entry
has to be finite afterwards (the Coriolis launch leaves structural zeros alone: it is compared starting from the zeros the
library hands it, and a second launch starting as NaN may leave unwritten only what is zero in the restatement).
`compared`, `refused` and `oracle_failed` count trees x precisions (a refused tree counts for both); `quantities` what was gated.

Gates (query_modes_ref.bound): fp64 1e-10, FD_CRB 1e-8; fp32 2e-5 for the kinematic / matrix modes and, for FD_CRB,
max(1e-3, 3 x r32) capped at 1e-2 with r32 the error of the REFERENCE'S formulation (the oracle's M, h and J on float32
arrays, a float32 numpy.linalg.solve) on the same state.  fp32 quantities above 1e-4 that are also more than 30 x r32 are
listed.  No GPU.  usage: python tools/fuzz/fuzz_query_modes.py [seed] [trials]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import helpers, query_emul, query_modes_ref as qm
import centroidal_ref as cr
import jaxsim_amd as ja
seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rng = np.random.default_rng(seed0)
trials = int(sys.argv[2]) if len(sys.argv) > 2 else 40
nfail = compared = quantities = refused = oracle_failed = 0; worst = {}; outliers = []; by_len = {}
def rec(mode, dtype, e, r32, tree, extra=''):
    global nfail, quantities
    quantities += 1
    key = mode + ('32' if dtype == np.float32 else '64')
    worst[key] = max(worst.get(key, 0), e)
    if dtype == np.float32 and r32 is not None:
        worst['FDCRB_r32'] = max(worst.get('FDCRB_r32', 0), r32)
        if qm.is_outlier(e, r32): outliers.append('  %s %s: %.2e, reference formulation in fp32 %.2e' % (mode, qm.tree_label(tree), e, r32))
    tol = qm.bound(mode, dtype, r32)
    if not (e < tol):
        nfail += 1; print('FAIL', key, '%.2e' % e, 'gate %.2e' % tol, 'r32 %s' % r32, qm.tree_label(tree), tree, extra)
trees = list(qm.FIXED_TREES) + [qm.draw_tree(rng, t, 9000 + t) for t in range(trials)]
for tree in trees:
    try:
        model = ja.JaxSimModel.build_from_model_description(qm.tree_text(tree))
        query_emul._setup(model, np.zeros((1, 1)), np.float32)  # (the packer: a tree it refuses is counted, not compared)
    except RuntimeError as ex:
        refused += 2; print('refused', qm.tree_label(tree), str(ex)[:90]); continue
    N = 3; n = model.dofs(); nL = model.number_of_links(); state_seed = int(rng.integers(0, 1000))
    I, O, code = (int(v) for v in rng.integers(0, 3, size=3))
    frames = qm.random_frames(model, rng)
    for dtype in (np.float64, np.float32):
        d0 = cr.random_data(model, N, seed=state_seed, dtype=dtype)  # (fixed bases: a non-zero stored base velocity)
        d64 = helpers.upcast(d0, model) if dtype == np.float32 else d0
        tau, f = helpers.random_inputs(model, N, state_seed + 1, dtype)
        try:
            with np.errstate(all='ignore'):
                ref = qm.truths(model, d64, tau.astype(np.float64), f.astype(np.float64), code, frames, I, O)
            if not all(np.all(np.isfinite(v)) for v in (ref['COR'], ref['M'], ref['FDCRB'])): raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            oracle_failed += 1; print('oracle_failed', qm.tree_label(tree)); continue
        compared += 1  # (per tree and precision, like oracle_failed; the quantities behind it are counted in `quantities`)
        block = helpers.odata_to_block(model, d0, dtype=dtype)
        R, J = query_emul.run_centroidal(model, block, jacobian=True, dtype=dtype)
        assert np.all(np.isfinite(R)) and np.all(np.isfinite(J)), ('centroidal: an entry was not written', tree)
        rec('CEN', dtype, qm.centroidal_error(model, d64, ref['CEN'], R.T.astype(np.float64), J.T.astype(np.float64).reshape(N, 6, 6 + n)), None, tree)
        blockI = helpers.odata_to_block(model, qm.with_rep(model, d0, qm.REPS[I]), dtype=dtype)
        e = 0.0
        for which, (P, H) in (('FRM_links', qm.fr.link_targets(model)), ('FRM_frames', frames)):
            R, J = query_emul.run_frames(model, blockI, P, H, I, O, jacobian=True, dtype=dtype)
            assert np.all(np.isfinite(R)) and np.all(np.isfinite(J)), ('frames: an entry was not written', tree)
            e = max(e, qm.frames_error(ref[which], R, J))
        rec('FRM', dtype, e, None, tree, (I, O))
        C, M = query_emul.run_coriolis(model, block, mass_matrix=True, fill=0.0, dtype=dtype)
        assert np.all(np.isfinite(C)) and np.all(np.isfinite(M))
        # a second launch that starts as NaN: what it leaves unwritten has to be a structural zero of the restatement
        Cn, Mn = query_emul.run_coriolis(model, block, mass_matrix=True, dtype=dtype)
        assert np.array_equal(np.nan_to_num(Cn), C) and np.array_equal(np.nan_to_num(Mn), M), ('coriolis: the two launches differ', tree)
        for got, want in ((Cn, ref['COR']), (Mn, ref['M'])):
            assert np.all(np.abs(want[np.isnan(got)]) < 1e-13 * max(1.0, np.abs(want).max())), ('coriolis: a non-zero entry was not written', tree)
        rec('COR', dtype, max(qm.rel(C, ref['COR']), qm.rel(M, ref['M'])), None, tree)
        out = query_emul.run_fd_crb(model, block, tau=tau.T, link_forces=f.reshape(N, -1).T, force_repr=code, dtype=dtype).T
        assert np.all(np.isfinite(out)), ('fd_crb: an entry was not written', tree)
        e = qm.rel(out, ref['FDCRB'])
        r32 = qm.fd_crb_fp32(model, d0, tau, f, code, ref['FDCRB']) if dtype == np.float32 else None
        rec('FDCRB', dtype, e, r32, tree, code)
        if dtype == np.float32 and 'n_links' in tree and tree['max_back'] == 1 and not tree['fixed_base']:
            b = by_len.setdefault(8 * ((nL + 7) // 8), [0.0, 0.0]); b[0] = max(b[0], e); b[1] = max(b[1], r32)
print('fp32 FD_CRB on floating serial chains (max_back 1), worst by length | the reference formulation in fp32 on the same states:')
for k, v in sorted(by_len.items()): print('  %2d .. %2d links  %.1e | %.1e' % (k - 7, k, v[0], v[1]))
print('fp32 quantities above 1e-4 AND more than 30 x what the reference\'s formulation loses in fp32 (the kernel\'s formulation, not the model): %d' % len(outliers))
for ln in outliers: print(ln)
print('fails', nfail, 'compared', compared, 'refused', refused, 'oracle_failed', oracle_failed, 'quantities', quantities, {k: '%.1e' % v for k, v in sorted(worst.items())})
