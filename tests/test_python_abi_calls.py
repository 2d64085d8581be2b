"""No GPU, no library.  What every Python wrapper passes across the C ABI, which exception it raises on a failing entry,
and the (restype, argtypes) of every key of capi.SIGNATURES equal tests/golden/python_abi_calls.json, entry by entry.
The JSON was recorded by tests/abi_call_cases.py at the commit before the binding was split into modules and is never
regenerated from refactored code (see that file's docstring)."""
import json
import os

import pytest

import abi_call_cases as acc


@pytest.fixture(scope="module")
def logs(golden_dir):
    with open(os.path.join(golden_dir, "python_abi_calls.json")) as f:
        golden = json.load(f)
    from dla_future_amd import capi
    before = capi._lib
    now = json.loads(acc.dumps(acc.record()))
    assert capi._lib is before, "the harness must leave capi._lib as it found it"
    return golden, now


@pytest.mark.parametrize("section", ["calls", "signatures", "structures"])
def test_wrappers_pass_what_the_recorded_binding_passed(logs, section):
    golden, now = logs
    assert sorted(now[section]) == sorted(golden[section])
    different = [k for k in golden[section] if now[section][k] != golden[section][k]]
    for k in different[:5]:
        print(f"{k}\n  recorded: {golden[section][k]}\n  now:      {now[section][k]}")
    assert not different, different


def test_the_log_is_deterministic_and_covers_the_public_names(logs):
    golden, now = logs
    assert acc.dumps(acc.record()) == acc.dumps(now)
    import dla_future_amd as daf
    from dla_future_amd import capi
    assert set(now["signatures"]) == set(capi.SIGNATURES)
    driven = {cid.split("[")[0].split(".")[0] for cid in now["calls"]}
    host_only = {"DLAFDescriptor", "LibraryNotBuilt", "lib", "lib_path", "make_descriptor", "type_char"}
    assert set(daf.__all__) - host_only <= driven, set(daf.__all__) - host_only - driven
