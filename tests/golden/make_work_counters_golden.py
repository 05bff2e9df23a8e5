#!/usr/bin/env python3
"""Records tests/golden/work_counters_single_workgroup.json on an MI355X: the cases of tests/work_counter_cases.py as the
commit BEFORE the work counter became two stages summed them (one workgroup, doc_terms.h work_count_kernel).

    python tests/golden/make_work_counters_golden.py [--package-root DIR] [--out FILE] [--commit HASH]

DIR: a checkout or copy whose pylda_amd (built) is recorded instead of this tree's; HASH: the commit DIR holds (kept in
the file as `recorded_from`).  Every case is run twice and must repeat itself exactly (the clock spans apart)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--out", default=os.path.join(HERE, "work_counters_single_workgroup.json"))
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.abspath(args.package_root))

from pylda_amd import _capi  # noqa: E402
import work_counter_cases as cases  # noqa: E402

record = {"recorded_from": args.commit}
for case in cases.CASES:
    out, again = cases.run(_capi, case), cases.run(_capi, case)
    record[case] = {field: out[field] for field in cases.FIELDS}
    assert record[case] == {field: again[field] for field in cases.FIELDS}, case
    assert all(float(v).is_integer() for v in record[case].values()), record[case]
    print(case, record[case], "clock spans", out["clock_spans"], flush=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", args.out, "from", os.path.dirname(_capi.__file__))
