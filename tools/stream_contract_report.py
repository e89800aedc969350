"""Prints the table of DESIGN.md section 7a: runs tests/test_stream_order.py on the GPU and reports, per entry point, how many warm
returns found the caller's stream still pending, with the calibrated sleep rate and the longest warm host time.

    python tools/stream_contract_report.py [pytest arguments]"""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


class Report:
    def pytest_sessionfinish(self, session):
        import stream_harness as sh
        print("\nSTREAM_CONTRACT " + json.dumps({"stats": sh.STATS, "observed": sh.OBSERVED}, sort_keys=True))
        for name in sh.header_stream_entry_points():
            o = sh.OBSERVED.get(name)
            says = "yes" if name in sh.SYNCHRONISING else "no"
            print(f"| `{name}` | {says} | " + ("-" if o is None else f"{o['pending']} of {o['pending'] + o['arrived']}") + " |")


if __name__ == "__main__":
    sys.exit(pytest.main(["-m", "gpu", os.path.join(REPO, "tests", "test_stream_order.py"), "-q", "-p", "no:cacheprovider", *sys.argv[1:]],
                         plugins=[Report()]))
