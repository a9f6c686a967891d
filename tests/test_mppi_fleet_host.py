"""CPU: `mppi.follow_fleet`'s shared-settings check on stub controllers -- one launch takes ONE parameter block and ONE maze
shape, so the controllers of a fleet must agree on them and the error names the first difference (no GPU, no library)."""
import types

import numpy as np
import pytest


def stub(T=8, K=20, lam=1.0, sigma=(3.0, 0.6), w_track=20.0, w_progress=0.5, w_collision=1.0e3, w_goal=50.0, window_back=8,
         window_fwd=56, shape=(20, 20), seed=0):
    params = types.SimpleNamespace(lam=lam, sigma=sigma, w_track=w_track, w_progress=w_progress, w_collision=w_collision,
                                   w_goal=w_goal, window_back=window_back, window_fwd=window_fwd, seed=seed)
    return types.SimpleNamespace(T=T, K=K, params=params, maze=np.zeros(shape, dtype=np.float32))


def test_controllers_that_agree_pass_whatever_their_seeds():
    from ditreeonlineplanner_amd import mppi
    mppi.check_fleet([stub(seed=s) for s in range(4)])
    mppi.check_fleet([stub()])
    with pytest.raises(ValueError, match="no controllers"):
        mppi.check_fleet([])


@pytest.mark.parametrize("change,name", [(dict(T=16), "T"), (dict(K=64), "K"), (dict(lam=2.0), "lam"), (dict(sigma=(3.0, 0.5)), "sigma"),
                                         (dict(w_track=1.0), "w_track"), (dict(w_progress=1.0), "w_progress"),
                                         (dict(w_collision=1.0), "w_collision"), (dict(w_goal=1.0), "w_goal"),
                                         (dict(window_back=4), "window_back"), (dict(window_fwd=4), "window_fwd"),
                                         (dict(shape=(20, 21)), "maze shape")])
def test_the_first_difference_is_named(change, name):
    from ditreeonlineplanner_amd import mppi
    with pytest.raises(ValueError, match=f"controller 2 differs from controller 0 in {name}:"):
        mppi.check_fleet([stub(), stub(seed=5), stub(**change), stub(T=32, K=99)])


def test_the_order_of_the_settings_decides_which_is_first():
    from ditreeonlineplanner_amd import mppi
    with pytest.raises(ValueError, match="controller 1 differs from controller 0 in K: 64 != 20"):
        mppi.check_fleet([stub(), stub(K=64, window_fwd=4, shape=(30, 30))])
