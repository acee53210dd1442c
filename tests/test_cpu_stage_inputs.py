"""The cases of tests/stage_inputs.py reach the stages they claim: the oracle alone, with the genuine NLopt, no GPU.  Conditions
on the generator, not measurements of the product: a failure here means a case has to be tuned (hpmvs_amd/synth.py moved a
histogram), never the condition.  tests/test_gpu_stage_parity.py compares the device with the oracle on the same cases; this
test keeps it from passing on inputs that have stopped reaching anything.  The measured histograms are in the docstring of
tests/stage_inputs.py."""
import pytest

import stage_inputs as si


@pytest.fixture(scope="module")
def oracle_runs():
    """Every case through the oracle, once: {case name: (kind, case, patches, acos-class count)}."""
    from oracle import oracle as orc
    orc.build()
    assert orc.best_optimizer() == orc.OPT_REF
    oscs, runs = {}, {}
    for kind, case, run in si.all_cases():
        if case.scene not in oscs:
            oscs[case.scene] = orc.OracleScene(si.scene(case.scene))
        osc = oscs[case.scene]
        inputs = si.expand_inputs(case, osc) if kind == "expand" else None
        patches = run(case, osc, inputs)
        runs[case.name] = (kind, case, patches, si.acos_class(lambda: run(case, osc, inputs)))
        print(f"{kind:6s} {case.name:20s} stages {si.histogram(p.stage for p in patches)}  nlopt {si.result_histogram(patches)}  "
              f"acos class {runs[case.name][3]}")
    return runs


def covered(runs, kind, required, name_part=""):
    """The stages of `required` that no case of the kind (and name) holds often enough."""
    best = {}
    for k, case, patches, _ in runs.values():
        if k == kind and name_part in case.name:
            for s, n in si.histogram(p.stage for p in patches).items():
                best[s] = max(best.get(s, 0), n)
    return {s: best.get(s, 0) for s, m in required.items() if best.get(s, 0) < m}


def test_case_sizes():
    """At most 12 views of 640 x 480 and 400 patches per case: the sizes of the existing small parity tests."""
    assert all(s["n_views"] <= 12 and (s["width"], s["height"]) == (640, 480) for s in si.SCENES.values())
    for kind, case, _ in si.all_cases():
        assert case.scene in si.SCENES
        n = case.args["n"] if kind != "expand" else case.args["n_parents"] * (6 if case.args["mode"] == 0 else 4)
        assert 0 < n <= 400, case.name
    assert len({c.name for _, c, _ in si.all_cases()}) == len(si.all_cases())


def test_every_case_reaches_its_minimum_counts(oracle_runs):
    for kind, case, patches, _ in oracle_runs.values():
        assert len(case.minimum) >= 2, case.name
        si.check_minimum(case, patches)


def test_no_case_leans_on_the_acos_exemption(oracle_runs):
    """The device rounds the start point's acos() to nearest, this host's libm not always: the GPU test lets one patch per case
    differ for that reason.  No case may hold more than one such patch."""
    for kind, case, _, changed in oracle_runs.values():
        assert changed <= 1, (case.name, changed)


def test_the_refine_cases_cover_the_late_stages(oracle_runs):
    assert covered(oracle_runs, "refine", si.REFINE_REQUIRED) == {}
    # some case holds >= 20 successes beside each late stage
    for stage in si.REFINE_REQUIRED:
        assert any(k == "refine" and si.histogram(p.stage for p in P).get(stage, 0) >= si.REFINE_REQUIRED[stage] and
                   si.histogram(p.stage for p in P).get(0, 0) >= 20 for k, _, P, _ in oracle_runs.values()), stage
    codes = set()
    for k, _, P, _ in oracle_runs.values():
        if k == "refine":
            codes |= set(si.result_histogram(P))
    assert codes >= si.NLOPT_RESULTS_REQUIRED, codes
    # stages 4 both ways: by image count (the optimiser never ran) and by NLopt's result code
    P4 = [p for k, _, P, _ in oracle_runs.values() if k == "refine" for p in P if p.stage == 4]
    assert sum(1 for p in P4 if p.nevals == 0) >= 5 and sum(1 for p in P4 if p.nlopt_result == -4) >= 1
    # no stage 5 anywhere (addImages only appends; overflow is 100)
    assert all(p.stage != 5 for _, _, P, _ in oracle_runs.values() for p in P)


def test_the_seed_loop_case_covers_its_exits(oracle_runs):
    assert covered(oracle_runs, "seed", si.SEED_LOOP_REQUIRED) == {}


@pytest.mark.parametrize("mode", ["extend", "branch"])
def test_the_expansion_cases_cover_late_stages_in_both_modes(oracle_runs, mode):
    assert covered(oracle_runs, "expand", si.EXPAND_REQUIRED, mode) == {}
    assert all(p.stage != 21 for k, c, P, _ in oracle_runs.values() if k == "expand" for p in P)
