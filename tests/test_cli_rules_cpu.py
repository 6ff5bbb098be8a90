"""The command line's option rules against their recordings (tests/cli_rules_lib.py, tests/golden/cli_rules/): every
recorded command line must end with the recorded status and the recorded stderr - the same refusal, in the same words,
and where a command line breaks several rules the same one of them - on the package's command line and on the one linked
against the stubs of the device library, where the "this library has no ..." lines are reached.  No case touches a GPU."""
import pytest

import cli_rules_lib as rules


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    return {"normal": rules.CLI, "stub": rules.build_stub(tmp_path_factory.mktemp("cli_rules"))}


def test_the_recordings_hold_the_generated_cases():
    want = {rules.shlex.join(args) for args in rules.cases()}
    assert len(want) > 1000
    for name in ("normal", "stub"):
        assert set(rules.load(name)) == want


@pytest.mark.parametrize("name", ["normal", "stub"])
def test_option_rules_replay(binaries, name):
    recorded = rules.load(name)
    got, usage = rules.run_all(binaries[name])
    assert usage == rules.load_usage()
    wrong = [(k, recorded[k], got[k]) for k in recorded if got[k] != recorded[k]]
    assert not wrong, f"{len(wrong)} of {len(recorded)} command lines differ, the first: {wrong[:3]}"


def test_the_stub_recording_reaches_the_missing_entry_points():
    texts = {t for _, t in rules.load("stub").values()}
    normal = {t for _, t in rules.load("normal").values()}
    assert sum("this library has no" in t for t in texts) >= 10
    assert not any("this library has no" in t for t in normal)
