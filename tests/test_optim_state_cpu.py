"""The shared optimizer state-dict helper (optim_state.py) against torch.optim.Adam(...).state_dict() of a three-tensor
module with one frozen parameter, with and without amsgrad, and the load-then-dump round trip."""
import numpy as np
import pytest
import torch

from crowdmod_ddpm_4d_amd import optim_state

NAMES = ("weight", "table", "bias")
HYPER = dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.003)


def _torch_state(amsgrad, steps=3):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5, 2), requires_grad=False),
          torch.nn.Parameter(torch.randn(4))]
    opt = torch.optim.Adam(ps, amsgrad=amsgrad, **HYPER)
    for k in range(steps):
        opt.zero_grad()
        ((ps[0] * ps[1][:4, :1]).sum() * (k + 1) + (ps[2] ** 2).sum()).backward()
        opt.step()
    return opt.state_dict()


@pytest.mark.parametrize("amsgrad", [False, True])
def test_dump_and_load_match_torch_adam(amsgrad):
    ref = _torch_state(amsgrad)
    keys = optim_state.AMSGRAD_KEYS if amsgrad else optim_state.ADAM_KEYS
    store = {}                                   # what a native handle holds: (name, which) -> float32 array
    step = optim_state.load(ref, NAMES, keys, lambda name, which, arr: store.__setitem__((name, which), arr))
    assert step == 3 and sorted(store) == sorted((n, w) for n in ("weight", "bias") for w in range(len(keys)))
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in store.values())
    got = optim_state.dump(NAMES, ("table",), keys, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"],
                           lambda name, which: store[(name, which)], step)
    assert list(got) == list(ref) == ["state", "param_groups"]
    assert list(got["state"]) == list(ref["state"]) == [0, 2]            # the frozen tensor keeps its position, without state
    for i, st in ref["state"].items():
        assert list(got["state"][i]) == list(st) == ["step"] + list(keys)
        assert got["state"][i]["step"].dtype == np.float32 and float(got["state"][i]["step"]) == float(st["step"]) == 3.0
        for key in keys:
            assert np.array_equal(got["state"][i][key], st[key].numpy()) and got["state"][i][key].shape == tuple(st[key].shape)
    assert len(got["param_groups"]) == 1
    g, r = got["param_groups"][0], ref["param_groups"][0]
    assert list(g) == list(r) and g == r and g["params"] == [0, 1, 2] and g["amsgrad"] is amsgrad
    # load-then-dump round trip of the helper's own output (numpy leaves, as a checkpoint read without torch gives them)
    again = {}
    assert optim_state.load(got, NAMES, keys, lambda name, which, arr: again.__setitem__((name, which), arr)) == 3
    assert sorted(again) == sorted(store) and all(np.array_equal(again[k], store[k]) for k in store)


def test_step_rules():
    keys = optim_state.ADAM_KEYS
    z = np.zeros(2, np.float32)
    # before the first update the optimizer holds no state; the group is complete all the same
    d = optim_state.dump(NAMES, ("table",), keys, 1e-3, (0.9, 0.999), 1e-8, 0.0, lambda n, w: z, 0)
    assert d["state"] == {} and d["param_groups"][0]["params"] == [0, 1, 2]
    assert optim_state.load({"state": {}}, NAMES, keys, None) == 0 and optim_state.load({}, NAMES, keys, None) == 0
    # the resumed step is the maximum over the entries, whatever their order and whatever holds the number
    opt = {"state": {2: {"step": torch.tensor(7.0), "exp_avg": z, "exp_avg_sq": z},
                     0: {"step": np.float32(5), "exp_avg": torch.zeros(2), "exp_avg_sq": z}}}
    seen = []
    assert optim_state.load(opt, NAMES, keys, lambda n, w, a: seen.append((n, w))) == 7
    assert seen == [("bias", 0), ("bias", 1), ("weight", 0), ("weight", 1)]
    opt["state"][0]["step"] = 23.0
    assert optim_state.load(opt, NAMES, keys, lambda n, w, a: None) == 23
