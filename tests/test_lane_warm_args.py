"""CPU-side checks of the switch that sends a batch's hot starts with new matrices and warm re-initialisations to the
lane-per-problem kernel (include/rsqp_hip_lane_warm.h, which include/rsqp_hip.h includes: rsqp_batch_set_lane_warm,
rsqp_batch_get_lane_warm): declared, exported, bound through a table of their own, and a null batch is an argument error before any
device call. The behaviour itself needs a GPU: tests/test_gpu_lane_warm.py. (That rsqp_describe_small_launch still reproduces every
golden plan -- the switch is a word its callers leave at 0 -- is tests/test_small_launch_plan.py's.)"""
from abi_cases import assert_entry_points

NEW = ("rsqp_batch_set_lane_warm", "rsqp_batch_get_lane_warm")


def test_entry_points_are_declared_exported_and_bound(capi):
    assert_entry_points(capi, "rsqp_hip_lane_warm.h", capi.LANE_WARM_SYMBOLS, NEW)
    assert callable(capi.Batch.set_lane_warm) and callable(capi.Batch.lane_warm)


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    assert L.rsqp_batch_set_lane_warm(None, 1) == capi.ERR_ARG
    assert L.rsqp_batch_set_lane_warm(None, 0) == capi.ERR_ARG
    assert L.rsqp_batch_get_lane_warm(None) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_the_launch_plan_words_do_not_name_the_switch(capi):
    """the switch is a batch's own: no word of rsqp_describe_small_launch carries it, and a plan described through that entry point
    never takes the warm build -- a hot start with new matrices of a batch the lane kernel takes stays on the 8-lane kernel there"""
    assert set(capi.LANE_WARM_SYMBOLS) == set(NEW)          # (the switch has its entry points ...)
    assert len(capi.SMALL_LAUNCH_IN) == 27 and len(capi.SMALL_LAUNCH_OUT) == 20
    assert not any("warm" in w for w in capi.SMALL_LAUNCH_IN + capi.SMALL_LAUNCH_OUT)
    words = dict(engine=-1, lanes=-1, waves=-1, no_tiny=0, lane=1, nq=200, nVmax=8, nCmax=2, mat_bytes_max=1024, mode=0, hbm=0,
                 state_engine=1, tiny_ok=1, uniV=8, uniC=2, uni_pat=1, desc=1, keep_state=1, skip_mark=1, member_mode=0, done_flag=0,
                 cert_out=0, x0=0, y0=0, guess_b=0, lane_hblock=8, uni_hreg=0)
    assert capi.describe_small_launch(**words)["family"] == 2
    for mode in (capi.MODE_HOT_MATRICES, capi.MODE_WARM_REINIT):
        plan = capi.describe_small_launch(**dict(words, mode=mode))
        assert plan["family"] == 1 and plan["mode"] == mode
    assert capi.describe_small_launch(**dict(words, member_mode=1))["family"] == 1
