"""CPU: every workspace-size query returns exactly the bytes recorded in tests/golden/workspace_sizes.json, so a change
to the host code that moves a slab, drops one or resizes one shows here, without a GPU (the queries are host-only)."""
import json

from tests.golden import make_workspace_sizes as gen


def test_workspace_sizes_are_pinned():
    want = json.load(open(gen.PATH))
    # spot values, so that a regenerated file cannot hide a change of all of them
    assert want["rollout B=15 N=10 H=50 fwd"] == 8244224 and want["rollout B=15 N=10 H=50 bwd"] == 22654976
    assert want["rollout B=110 N=1 H=256 keep=0 fwd"] == 11275776
    assert want["rollout B=110 N=1 H=256 keep=0 bwd"] == 35056128
    assert (want["lstm B=110 H=256 fwd"], want["lstm B=110 H=256 bwd"]) == (12416256, 73468672)
    assert want["cell hook B=129 H=200 layer0=1"] == 1277184
    got = gen.measure()
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}
