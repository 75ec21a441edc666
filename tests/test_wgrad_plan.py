"""The weight-gradient planner (csrc/kernels/wgrad_plan.cpp: which kernel, tile and split count a
convolution's weight gradient gets, and which convolutions go to the library) decides today what
tests/data/wgrad_plans.txt records, line for line.  Host-only: the planner is compiled with the C++
compiler into build/wgrad_plan_dump (tests/native/wgrad_plan_dump.cpp) and needs no GPU."""
import subprocess

from conftest import ROOT

FIXTURE = ROOT + "/tests/data/wgrad_plans.txt"


def _rows():
    with open(FIXTURE) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]


def _field(row, name):
    """The value of ``name=`` in a fixture row's answer, or None."""
    for tok in row.split(" -> ", 1)[1].split():
        if tok.startswith(name + "="):
            return tok[len(name) + 1:]
    return None


def test_planner_matches_recorded_plans():
    subprocess.check_call(["make", "-C", ROOT, "-s", "build/wgrad_plan_dump"])
    with open(FIXTURE) as f:
        r = subprocess.run([ROOT + "/build/wgrad_plan_dump"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:]
    got, want = r.stdout.splitlines(), _rows()
    assert len(got) == len(want)
    diff = ["-%s\n+%s" % (w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d of %d rows differ:\n%s" % (len(diff), len(want), "\n".join(diff[:20]))


def test_fixture_covers_every_route_and_kernel():
    """A shortened fixture cannot hide a family: every route outcome and every kernel is recorded at least
    once among the route rows, every kernel and both kinds of refusal among each family's explicit plans."""
    rows = _rows()
    routes = [r for r in rows if r.startswith("route ")]
    assert {_field(r, "route") for r in routes} == {"library", "square", "rect"}
    kernels = {"Tiled", "Rows3x3", "RowsRect", "RowsRing"}
    assert {(_field(r, "route"), _field(r, "kernel")) for r in routes} == {
        ("library", None), ("square", "Tiled"), ("square", "Rows3x3"), ("rect", "Tiled"), ("rect", "RowsRect"),
        ("rect", "RowsRing")}
    assert {_field(r, "cap") for r in routes if _field(r, "route") != "library"} == {str(1 << 23), str(1 << 31)}
    square = [r for r in rows if r.startswith("plan square ")]
    rect = [r for r in rows if r.startswith("plan rect ")]
    assert {_field(r, "kernel") for r in square + rect} - {None} == kernels
    assert {r.split()[2] for r in square} == {str(v) for v in range(-1, 8)}
    assert {r.split()[2] for r in rect} >= {str(v) for v in range(-1, 14)}
    for msg in ("tile/channel mismatch", "rows variant needs 3x3/s1"):
        assert any(r.endswith("error: conv_wgrad: " + msg) for r in square), msg
    assert any("error: conv_wgrad_rect: row-image variant unsupported" in r for r in rect)
    assert len(rows) >= 200
