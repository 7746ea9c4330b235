"""CPU: the launch-form queries answer every request of a fixed grid as the pinned table says (tests/golden/launch_forms.json,
written by tools/launch_forms.py from the build named in the file).  The launch-plan compiler sizes workspaces, hands out
tile counters and patches producers on these answers, so a change of ANY answer is a change of behaviour: regenerate the
fixture only together with a measured reason."""
import json

from tools import launch_forms as LF


def test_every_query_answers_as_the_pinned_table():
    fx = json.load(open(LF.FIXTURE))
    reqs = LF.requests()
    assert fx["columns"] == LF.COLUMNS and fx["grid"] == LF.grid_digest(reqs) and len(fx["rows"]) == len(reqs) <= 6000
    LF.check_discriminates(reqs, fx["rows"])
    rows = LF.table(LF.L.lib(), reqs, with_ctr=False)
    bad = [(LF.describe(r), want[:-1], got[:-1]) for r, want, got in zip(reqs, fx["rows"], rows) if want[:-1] != got[:-1]]
    for d, want, got in bad[:20]:
        print("%s\n  pinned  %s\n  library %s" % (d, want, got))
    assert not bad, "%d of %d requests answered differently (columns %s)" % (len(bad), len(reqs), LF.COLUMNS[:-1])
