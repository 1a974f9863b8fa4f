"""CPU: every refusal of the fourteen neighbour-search entry points -- return code and message, byte for byte, and which of two
bad arguments speaks first -- against tests/golden/knn_refusals.json, the transcript tools/record_knn_refusals.py wrote from the
library of the commit BEFORE the three searches were moved onto one host shell.  The library loads without a GPU and a refused call
launches nothing; the replay stops at the first call that is not refused."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_refusals.json")


def test_every_recorded_refusal_is_repeated_word_for_word():
    import __graft_entry__ as ge
    ge.build()
    from slnlp import _lib
    spec = importlib.util.spec_from_file_location("record_knn_refusals", os.path.join(ROOT, "tools", "record_knn_refusals.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(GOLDEN) as f:
        recorded = json.load(f)
    entries = {name for name in _lib.SIGNATURES if name.startswith(("slnlp_edit_", "slnlp_field_"))}
    assert len(entries) == 14 and set(recorded["entries"]) == entries == {c["entry"] for c in recorded["cases"]}
    assert len(recorded["cases"]) >= 400 and all(c["rc"] != 0 for c in recorded["cases"])
    got = tool.replay(_lib.load(), recorded)
    assert len(got) == len(recorded["cases"])
    for want, now in zip(recorded["cases"], got):
        assert now == want
    # the recorder's own cases are the file's: a case added to the tool is recorded before it counts
    assert [(e, n) for e, n, _ in tool.cases()] == [(c["entry"], c["case"]) for c in recorded["cases"]]
