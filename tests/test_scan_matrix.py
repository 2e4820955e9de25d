"""The keyed index scans on the CPU: HostCache's matcher x action matrix (the semantic
reference of k_keyed_scan / k_list_scan) against the Python model of tests/scan_matrix_cases.py."""
import pytest

import scan_matrix_cases as sm


@pytest.mark.parametrize("matcher,kind", sorted(sm.CASES))
def test_host_scan_matrix(matcher, kind):
    sm.run_case(["cpu"], matcher, kind)
