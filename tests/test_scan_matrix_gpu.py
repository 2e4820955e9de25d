"""The keyed index scans on the GPU: every instance of k_keyed_scan<Matcher, Action> and of
k_list_scan<Matcher> against the host twin and the Python model of tests/scan_matrix_cases.py."""
import pytest

import scan_matrix_cases as sm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("matcher,kind", sorted(sm.CASES))
def test_twin_scan_matrix(cuda_dev, matcher, kind):
    sm.run_case([cuda_dev, "cpu"], matcher, kind)
