"""The oracle's six libraries reproduce, bit for bit, the outputs recorded in tests/golden/oracle_digests.json: frames, listed pixels,
bounce counts, atmosphere cubes, post-process, the micro entry points, the margins build's planes, and the witness build idle, under
every base variant, perturbation, ensemble member, replay and search (tests/golden/record_oracle_digests.py says what is digested and
how the fixture was recorded: from the oracle as it stood before oracle/pt_oracle.c was split into the contract and the study builds under
oracle/study/).  A digest that moves means an oracle library no longer computes what it computed."""
import importlib.util
import json
import os

import pytest

import __graft_entry__ as graft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_oracle_digests", os.path.join(GOLDEN, "record_oracle_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(recorder):
    with open(recorder.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed(recorder):
    return recorder.compute(graft.load_oracle())


def test_every_recorded_digest_is_reproduced(recorded, computed):
    assert sorted(computed) == sorted(recorded), "the set of digested outputs changed: re-record deliberately or restore the entry point"
    moved = sorted(k for k in recorded if computed[k] != recorded[k])
    assert not moved, f"{len(moved)} of {len(recorded)} oracle outputs changed, e.g. {moved[:8]}"


def test_fixture_covers_every_library_and_study_knob(recorded, recorder):
    for kind in recorder.KINDS:
        for what in ("render_frame", "render_pixels", "bounce_counts", "atmosphere", "postprocess", "micro", "stubs"):
            assert any(k.startswith(f"{kind}/{what}") for k in recorded), (kind, what)
    for bits in (7, 951, 1, 2, 4, 128, 256, 512, 8, 16, 24, 32, 64):
        assert any(k.startswith(f"perturb/base{bits}/render_frame") for k in recorded) and f"perturb/base{bits}/atmosphere/16" in recorded, bits
    for what in ("unfused", "signature", "nan_env", "close_decisions", "pixel_variant", "witness_search", "llvmpipe_like", "ensemble1", "ensemble2",
                 "ensemble12345", *(f"perturbation{p}{u:+d}" for p in range(7) for u in (1, -1))):
        assert any(k.startswith(f"perturb/{what}") for k in recorded), what
    assert any(k.startswith("margins/planes") for k in recorded) and any(k.startswith("margins/pixels") for k in recorded)
    assert all(len(v) == 64 and set(v) <= set("0123456789abcdef") for v in recorded.values()), "the fixture holds names and hex digests only"


def test_idle_witness_and_margins_builds_equal_the_contract(recorded):
    """with no knob set the witness library, and always the margins library's image, are the contract's (the fixture says so itself)"""
    shared = [k[len("contract/"):] for k in recorded if k.startswith("contract/") and not k.startswith("contract/stubs")]
    assert len(shared) > 10
    for what in shared:
        assert recorded[f"perturb/{what}"] == recorded[f"contract/{what}"], what
        assert recorded[f"margins/{what}"] == recorded[f"contract/{what}"], what
