"""csrc/inflx_sf.h at its seams, limits and tiny arguments, on the host: the whole table of tests/special_cases.py through the
host build of the header (tests/sf_host.cpp) and through the table's verdict.  tests/test_special_edges_gpu.py runs the same
table, with the same verdict, through the header inside a gfx950 program."""

import pytest
import special_cases as sc
from test_special_functions import sf  # noqa: F401  (the host build of the header: one recipe)

COUNTS = {"seams": 2075, "range": 10433, "tiny": 598, "limits": 141, "status": 211}


@pytest.fixture(scope="module")
def run(sf):  # noqa: F811
    table = sc.table(sf)
    results, status = sc.run_on_host(sf, table)
    verdicts = sc.judge(table, results, status, device=False)
    print(sc.report(table, verdicts, "csrc/inflx_sf.h built for the host (g++ -ffp-contract=off, glibc) against mpmath"))
    return table, verdicts, status


def test_the_table_holds_every_case(run):
    table, verdicts, _ = run
    assert table.counts() == COUNTS
    # nothing is left out: every case has a verdict, and escapes its budget by one of the stated rules only
    assert len(verdicts) == len(table.cases) and all(v.rule in sc.RULES for v in verdicts)
    assert not [c for c, v in zip(table.cases, verdicts) if v.rule == "declined" and not c.decline_ok]
    assert not [c for c, v in zip(table.cases, verdicts) if v.rule in sc.LENIENT and c.check != "budget"]
    # the 2F0 seams were found: one pair for every parameter pair whose series does not terminate
    assert sum(c.family == "seams" and c.fn == "2F0" for c in table.cases) == 2 * (len(sc.SEAM_2F0) - 1)


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_header_on_the_host(run, family):
    table, verdicts, status = run
    bad = sc.failures(table, verdicts, family) + sc.status_failures(table, status, family)
    assert not bad, f"{len(bad)} of the {family} cases fail:\n" + "\n".join(bad[:60])
