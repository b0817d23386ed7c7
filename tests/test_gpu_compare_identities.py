"""The identities of tests/test_compare_identities_cpu.py with the kernels: s2s_sdtw_kernel held to s2s_dtw_kernel<false> by the
brute force over all intervals of the target (one launch of up to 820 pairs at band L per problem), and s2s_dtw_kernel<false> /
<true> with s2s_dtw_trace_kernel against the host entries at extreme slopes, every pair alone and all pairs of one band in one
launch.  Every check is an equality of integers."""
import pytest

from test_compare_identities_cpu import BRUTE_SHAPES, check_brute_force, check_slopes
from test_compare_open_ends_cpu import KINDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,H", BRUTE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sdtw_is_the_minimum_over_all_intervals(kind, L, H):
    check_brute_force(kind, L, H, cpu=False)


def test_slopes_alone_and_in_one_launch():
    check_slopes(cpu=False)
