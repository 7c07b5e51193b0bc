"""CPU tests of the constructed class tables of tests/emedge_corpus.py (the EM plan's record, window and tile edges): the tables keep
the builder's invariants, what each case promises by hand agrees with the numpy model of the plan's rules, and on every table the C
oracle and the numpy restatement agree with the 50-digit mpmath restatement after 1, 2 and 5 iterations, EM and VBEM.  The oracle's
own distance to mpmath is recorded per case (printed; the device's bound in tests/test_gpu_emedges.py is 8 x that distance).

The runs to convergence demand EQUAL stop iterations of the device, which is fair only where the stop test is not a coin toss:
max_rel_diff at the stop iteration, and at the one before it, differs from tol by more than 1e-6 relative -- checked here on the
oracle for every table (the tables' seeds were picked so that it holds)."""
import numpy as np
import pytest

import em_numpy_restatement as R
import emedge_corpus as EC

NAMES = sorted(EC.CASES)
TOL = 0.01


@pytest.mark.parametrize("name", NAMES)
def test_corpus_invariants_and_promised_plan_facts(name):
    """labels sorted, duplicate free, distinct, canonical order; the facts the case states by hand are what the plan's rules give"""
    case = EC.CASES[name]()
    EC.check_invariants(case)
    model = EC.plan_model(case["rowptr"], case["ids"])
    if case["expect"].get("renumbered"):
        # (the model describes the caller's order: here it must show why the plan tries an order of its own)
        assert len(case["counts"]) >= EC.K_RENUMBER_MIN and model["E"] * 8 > int(case["rowptr"][-1])
        return
    for k, v in case["expect"].items():
        assert model[k] == v, (name, k, v, model[k])
    if name.startswith("renumber_gate"):
        assert len(case["counts"]) == EC.K_RENUMBER_MIN - 1 and model["E"] * 8 > int(case["rowptr"][-1])


def test_renumber_gate_tables_differ_by_one_class():
    a, b = EC.CASES["renumber_gate_4095"](), EC.CASES["renumber_gate_4096"]()
    assert len(a["counts"]) == 4095 and len(b["counts"]) == 4096
    assert np.array_equal(a["rowptr"], b["rowptr"][:-1]) and np.array_equal(a["ids"], b["ids"][:len(a["ids"])])


def test_record_size_tables_differ_by_one_class_and_in_parity():
    a, b = EC.CASES["record_sizes_even"](), EC.CASES["record_sizes_odd"]()
    assert len(a["counts"]) % 2 == 0 and len(b["counts"]) == len(a["counts"]) + 1
    k = np.diff(a["rowptr"].astype(np.int64))
    assert sorted(set(k.tolist())) == sorted(EC.REC_SIZES) and all(int(np.sum(k == s)) >= 3 for s in EC.REC_SIZES)


def test_crowded_tile_model_redoes_the_plan():
    """the one large table (GPU test only: the oracle is its reference) -- here only that the plan's rules redo it, for several CU counts"""
    for n_cu in (256, 304):
        case = EC.crowded_tile(n_cu)
        m = EC.plan_model(case["rowptr"], case["ids"], n_cu=n_cu)
        assert int(case["rowptr"][-1]) > 2 * n_cu * EC.K_TILE_CLS and m["redone"] >= 1 and m["most_classes"] <= EC.K_TILE_CLS
        for k, v in case["expect"].items():
            assert m[k] == v, (k, v, m[k])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_numpy_agree_with_mpmath_and_record_the_yardstick(built, name):
    """1, 2 and 5 iterations, EM and VBEM: the oracle and the numpy restatement against mpmath (1e-11, as tests/test_em_independent.py
    holds them on its toys); the supports are equal and no value sits at the truncation cut-off; the oracle's distance is printed"""
    case = EC.CASES[name]()
    ref = EC.reference(name, case)
    with np.errstate(all="ignore"):                       # (a zero-count class's stored weights are 0 / 0, as in the reference)
        p = R.Problem(case["eff"], case["rowptr"], case["ids"], case["counts"], case["num_mapped"])
    for vb, r in ref.items():
        a = p.alpha0()
        done = 0
        for n in EC.FIXED_ITERS:
            with np.errstate(all="ignore"):
                while done < n: a = p.step(a, vb); done += 1
            f = r["fixed"][n]
            assert EC.clear_of_cutoff(f["mp_raw"], vb), (name, vb, n)
            d_np = EC.rel_dist(EC.truncate(a, vb), f["mp"])
            print(f"{name} {'VBEM' if vb else 'EM'} n={n}: oracle-mpmath {f['dist']:.3e} numpy-mpmath {d_np:.3e} device bound {EC.bound_for(f['dist']):.3e}")
            assert f["dist"] <= 1e-11 and d_np <= 1e-11
            assert f["stats"]["iters"] == n and f["stats"]["n_active"] == p.n_active
        for t in case.get("truncated", ()):
            assert r["fixed"][5]["mp"][t] == 0.0 and p.active[t], (name, t)


@pytest.mark.parametrize("name", NAMES)
def test_stop_iteration_is_not_a_coin_toss(built, name):
    """at the oracle's stop iteration and at the one before it max_rel_diff is more than 1e-6 (relative) away from tol; and the
    converged oracle against the recorded mpmath result of the same iteration"""
    ref = EC.reference(name)
    for vb, r in ref.items():
        c = r["conv"]
        st, prev = c["stats"], c["prev_stats"]
        assert st["iters"] >= 50 and prev["iters"] == st["iters"] - 1
        for s in (st, prev):
            assert abs(s["max_rel_diff"] - TOL) > 1e-6 * TOL, (name, vb, s)
        assert st["converged"] and st["max_rel_diff"] <= TOL
        assert st["iters"] == 50 or prev["max_rel_diff"] > TOL
        assert EC.clear_of_cutoff(c["mp_raw"], vb)
        print(f"{name} {'VBEM' if vb else 'EM'} converged at {st['iters']}: oracle-mpmath {c['dist']:.3e} device bound {EC.bound_for(c['dist']):.3e}")
        assert c["dist"] <= 1e-11


def test_zero_count_class_of_several_members_is_nan_under_vbem_in_the_oracle(built):
    """the contract of include/sfgpu.h for count 0 rests on this: VBEMUpdate_ (:340-361) has no isnan guard, so the reference -- and the
    oracle, which follows it -- returns NaN for such a class; EM (:269) skips it.  The kernels skip it in both modes."""
    from oracle import oracle as O
    case = EC.CASES["extremes_zero_counts"]()
    args = (case["eff"], case["rowptr"], case["ids"], case["counts"], case["num_mapped"])
    _, a_vb, _, _ = O.em_optimize(*args, use_vbem=True, tol=0.0, min_iter=1, max_iter=1)
    _, a_em, _, _ = O.em_optimize(*args, use_vbem=False, tol=0.0, min_iter=1, max_iter=1)
    assert np.isnan(a_vb).any() and np.isfinite(a_em).all()
    with pytest.raises(ValueError):
        R.optimize_mp(case["eff"], case["rowptr"].astype(np.int64), case["ids"], case["counts"], case["num_mapped"], vb=True, n_iter=1)
