"""CPU: the host chains of tests/list_frame_cases.py are worth comparing a device against -- a census of what the three recipes' four
frames exercise, asserted on the reference alone, and the comparison helper of the GPU test rejecting one flipped byte.  No GPU code
is touched: every stage runs through its host twin."""
import numpy as np
import pytest

import list_frame_cases as fc
import list_upsample_cases as lu
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
RECIPES = sorted(fc.RECIPES)


def frames_of(name):
    R = fc.RECIPES[name]
    return R, fc.host_chain(name), [fc.Frame(R, k) for k in range(fc.FRAMES)]


def lengths_of(name, state):
    return state["hlen"] if name == "C" else state["mlen"]


@pytest.mark.parametrize("name", RECIPES)
def test_histories_grow_to_the_frame_count_and_the_moving_box_resets_some(name):
    R, chain, _ = frames_of(name)
    last = lengths_of(name, chain[-1])
    assert last.max() == fc.FRAMES and (last == fc.FRAMES).sum() > 100, "no history survives the four frames"
    for k, state in enumerate(chain):
        n = lengths_of(name, state)
        assert n.max() == k + 1
    still = lengths_of(name, fc.host_chain(name, still_box=True)[-1])
    assert ((last == 1) & (still == fc.FRAMES)).any(), "no active pixel's history is reset to 1 by the moving box"
    assert (chain[-1]["pts"][..., 3] == 2).sum() > 20, "the moved box is hardly on screen"
    assert (last[:, chain[-1]["pts"][..., 3] == 2] == fc.FRAMES).any(), "the chain does not follow the moving box"


@pytest.mark.parametrize("name", RECIPES)
def test_the_image_has_many_values_and_changes_from_frame_to_frame(name):
    R, chain, _ = frames_of(name)
    for k, state in enumerate(chain):
        assert len(np.unique(state["rgb"].reshape(-1, 3), axis=0)) > 32, (k, "the image is nearly flat")
        if k:
            assert (state["rgb"] != chain[k - 1]["rgb"]).mean() > 0.05, (k, "two consecutive frames are nearly the same image")


def test_recipe_a_retraces_few_pixels_and_takes_no_fallback():
    R, chain, frames = frames_of("A")
    phases = set()
    for state, f in zip(chain, frames):
        phases.add((int(f.up.phase_x), int(f.up.phase_y)))
        share = (state["keep"] != 0).mean()
        assert 0.0 < share < 0.5, (f.k, "the retrace map marks", share)
        want, fallback = lu.upsample_rule(R.count, False, f.up, state["pos"], state["nrm"], state["lpos"], state["lnrm"], state["lo"],
                                          state["map"], state["lmap"], keep=state["keep"], before=state["counts"])
        assert (fallback == 0).all(), (f.k, "a written byte came from the fallback")
        assert (want == state["counts"]).all(), (f.k, "the host upsample disagrees with the numpy rule")
        assert state["counts"].max() == 16 and (state["counts"][1] <= 1).all()
    assert len(phases) == 4, "the phase does not rotate through a quad"


def test_recipe_a_the_clamp_and_the_propagated_variance_matter():
    R, chain, frames = frames_of("A")
    clamped = propagated = False
    for state, f in zip(chain[1:], frames[1:]):
        prev = state["prev_g"] + state["prev_m"]
        plain = api.accumulate_moments_soft_light_list(f.lights, f.tp, state["pos"], state["nrm"], state["counts"], prev, state["map"],
                                                       motion=(state["pts"], state["pnr"]))
        clamped |= any((a != b).any() for a, b in zip(plain[:2], (state["mean"], state["square"])))
        assert (plain[2] == state["mlen"]).all(), "the clamp shortened a history"
        guided = api.wide_filter_guided_temporal_mean_soft_light_list(
            f.lights, api.WideGuideTemporalParams.make(3, 12, 2, fc.NORMAL_COS, fc.PLANE_EPS), state["pos"], state["nrm"], state["counts"],
            (state["mean"], state["square"], state["mlen"]), state["map"])
        propagated |= bool((guided.view(u32) != state["vis"].view(u32)).any())
    assert clamped, "the clamped moments equal the unclamped ones in every frame"
    assert propagated, "the propagated filter equals the guided temporal mean filter in every frame"


def test_recipe_b_takes_fallbacks_and_its_last_pass_accepts_taps():
    R, chain, frames = frames_of("B")
    for state, f in zip(chain, frames):
        want, fallback = lu.upsample_rule(R.count, False, f.up, state["pos"], state["nrm"], state["lpos"], state["lnrm"], state["lo"],
                                          state["map"], state["lmap"])
        assert (fallback != 0).sum() > 10, (f.k, "no pixel takes the fallback")
        assert (want == state["counts"]).all(), (f.k, "the host upsample disagrees with the numpy rule")
        four = api.wide_filter_guided_temporal_mean_soft_light_list(
            f.lights, api.WideGuideTemporalParams.make(4, 12, 2, fc.NORMAL_COS, fc.PLANE_EPS), state["pos"], state["nrm"], state["counts"],
            (state["mean"], state["square"], state["mlen"]), state["map"])
        assert (four.view(u32) != state["vis"].view(u32)).any(), (f.k, "no tap 16 pixels away is accepted: the fifth pass is a copy")


def test_recipe_c_the_clamp_changes_the_history_and_every_bit_is_set_and_clear():
    R, chain, frames = frames_of("C")
    changed = False
    for state, f in zip(chain, frames):
        for l in range(8):
            bit = (state["mask"] >> l) & 1
            assert bit.any() and not bit.all(), (f.k, l, "a light's bit is constant over the mask")
        if f.k:
            plain = api.accumulate_visibility_list(f.hard, f.tp, state["pos"], state["nrm"], state["vis"], state["prev_g"] + state["prev_h"],
                                                   state["map"], motion=(state["pts"], state["pnr"]))
            changed |= bool((plain[0].view(u32) != state["hvis"].view(u32)).any())
            assert (plain[1] == state["hlen"]).all()
    assert changed, "the clamp never changes the history"


# ------------------------------------------------------------------------------------------------------------ the comparison helper
def as_buffers(R, state, preset=fc.PRESET_DEVICE):
    """The host state as a device run would be read back: payload bytes, the count planes in buffers of eight planes, the low-resolution
    ones in buffers of the largest phase, the rest holding the preset."""
    size = {"lpos": fc.LO * 16, "lnrm": fc.LO * 16, "lmap": fc.LO, "lo": R.count * fc.LO}
    planes8 = {"counts": 1, "mean": 2, "square": 4, "mlen": 1, "vis": 4, "hvis": 4, "hlen": 1}
    out = {}
    for name in fc.PLANES[R.name]:
        raw = np.ascontiguousarray(state[name]).reshape(-1).view(np.uint8)
        buf = np.full(max(raw.size, size.get(name, 0), 8 * fc.N * planes8.get(name, 0)), preset, np.uint8)
        buf[:raw.size] = raw
        out[name] = buf
    return out


@pytest.mark.parametrize("name", RECIPES)
def test_the_comparison_accepts_the_chain_itself_and_rejects_one_flipped_byte(name):
    R, chain, _ = frames_of(name)
    for k, state in enumerate(chain):
        fc.compare_frame(R, as_buffers(R, state), state, (name, k))
    state = chain[2]
    for plane in fc.PLANES[name]:
        got = as_buffers(R, state)
        got[plane][np.ascontiguousarray(state[plane]).nbytes // 2] ^= 0x01
        with pytest.raises(AssertionError, match=plane):
            fc.compare_frame(R, got, state, (name, 2))
    got = as_buffers(R, state)
    got["vis"][-1] ^= 0x80                                                # behind plane count - 1 (A) or in the last plane (B, C)
    with pytest.raises(AssertionError, match="vis"):
        fc.compare_frame(R, got, state, (name, 2))


def test_a_flipped_byte_of_one_intermediate_plane_is_rejected_there_and_downstream():
    """One defined byte of one intermediate plane -- a count byte of recipe A's light 0 behind the upsample of frame 1 -- flipped inside
    the host runner: the comparison rejects the count planes, and, with that plane put right again, the moments made from it; the
    flip reaches the next frame's moments through the history."""
    R = fc.RECIPES["A"]
    truth = fc.host_chain("A")
    y, x = np.argwhere(((truth[1]["map"] & 1) != 0) & (truth[1]["counts"][0] == 2))[0]

    def flip(h):
        h["counts"][0, y, x] ^= 1

    h = fc.new_host_state()
    fc.run_host_frame(R, h, fc.Frame(R, 0))
    fc.compare_frame(R, as_buffers(R, h), truth[0], "frame 0")
    fc.run_host_frame(R, h, fc.Frame(R, 1), perturb=("upsample", flip))
    got = as_buffers(R, h)
    with pytest.raises(AssertionError, match="counts"):
        fc.compare_frame(R, got, truth[1], "frame 1")
    assert (h["counts"] != truth[1]["counts"]).sum() == 1
    got["counts"] = as_buffers(R, truth[1])["counts"]
    with pytest.raises(AssertionError, match="mean"):
        fc.compare_frame(R, got, truth[1], "frame 1, the count planes put right")
    fc.run_host_frame(R, h, fc.Frame(R, 2))
    with pytest.raises(AssertionError, match="mean"):
        fc.compare_frame(R, as_buffers(R, h), truth[2], "frame 2")
