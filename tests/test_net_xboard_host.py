"""CrossBoardRiseV3 on the host: parameter names and shapes against the hand-written list of the reference class
(tests/golden/crossboard_state_dict.json), and checkpoint ingestion choosing the model by its cross_board_blocks. keys."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crossboard_state_dict.json")


@pytest.mark.parametrize("layers", [1, 2])
def test_state_dict_names_and_shapes(layers):
    from hivemind_amd import net as N
    want = json.load(open(GOLDEN))[str(layers)]
    got = {k: list(v.shape) for k, v in N.CrossBoardRiseV3(attention_layers=layers).state_dict().items()}
    assert got == want


@pytest.mark.parametrize("layers", [0, 1, 2])
def test_load_checkpoint_picks_the_model(tmp_path, layers):
    """layers = 0: a plain RISEv3 checkpoint still loads as RiseV3."""
    from hivemind_amd import net as N
    model = N.cross_board_rise_v33(layers) if layers else N.rise_v33()
    path = tmp_path / "ckpt.tar"
    torch.save({"model_state_dict": model.state_dict(), "optimizer_state_dict": {}}, path)
    loaded = N.load_checkpoint(str(path))
    assert type(loaded) is (N.CrossBoardRiseV3 if layers else N.RiseV3)
    if layers:
        assert len(loaded.cross_board_blocks) == layers
    for k, v in model.state_dict().items():
        assert torch.equal(loaded.state_dict()[k], v)
