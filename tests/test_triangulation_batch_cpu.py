"""olf_search_for_triangulation_batch_dev without a device: the argument checks come before anything touches one."""
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib


def test_null_context_is_refused():
    assert lib().olf_search_for_triangulation_batch_dev(None, None, None, 2, 1, None, None, None, 0, 1, 4, None, None, None) == OLF_ERR_INVALID
    assert "olf_search_for_triangulation_batch_dev" in last_error()
