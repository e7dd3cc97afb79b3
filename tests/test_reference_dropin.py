"""The INTEGRATION.md drop-in against the reference's call sites, self-contained: what the reference's code does with
this package's objects is driven here through the interface it uses, and compared with what the reference itself
wrote (golden fixtures, tests/golden/gen_golden.py).

Checked: (1) the reference's TrainingDataStorage.save (data.py:52-64, storage.py:12-17) can take this package's
GameData objects -- their `.data` reduce with np.sum, the boards mirror and encode through create_fliplr / to_array
(native_to_pytorch, data.py:78-105, add_fliplr=True) -- and the data.pth tensors equal those the reference wrote for
its own objects, the games.pkl pickle round-trips; (2) the W/D/L count of training.py:137-141, with the reference's
Result members (reference_result.json), works on this package's results."""
import enum
import os
import pickle

import numpy as np

from conftest import load_json, load_npz


def _mirror_games():
    from connect4_amd.board import Board
    from connect4_amd.training_game import GameData
    from connect4_amd.utils import Result
    games = []
    for g in load_json("selfplay_net.json"):
        gd = GameData()
        for bb, mv, v, p in zip(g["boards"], g["moves"], g["values"], g["policies"]):
            gd.add_move(Board.from_bits(*bb), mv, v, np.array(p))
        gd.result = Result(g["result"])
        games.append((g["name"], gd))
    return games


def _storage_save(games, folder):
    """The reference writer's use of the games it is given: pickle the list, reduce their TrainingData with np.sum,
    append the left-right mirrored boards / reversed priors / repeated values, float32 tensors into data.pth."""
    import torch
    with open(os.path.join(folder, "games.pkl"), "wb") as f:
        pickle.dump(games, f)
    data = np.sum([g.data for g in games])
    boards = list(data.boards) + [b.create_fliplr() for b in data.boards]
    values = np.concatenate([np.asarray(data.values), np.asarray(data.values)])
    priors = list(data.priors) + [np.flip(p) for p in data.priors]
    torch.save({"boards": torch.tensor(np.array([b.to_array() for b in boards]), dtype=torch.float32),
                "values": torch.tensor(values, dtype=torch.float32),
                "priors": torch.tensor(np.array(priors), dtype=torch.float32)}, os.path.join(folder, "data.pth"))


def test_reference_storage_accepts_mirror_game_data(tmp_path):
    import torch
    npz = load_npz("selfplay_net_tables.npz")
    for name, gd in _mirror_games():
        folder = os.path.join(str(tmp_path), name)
        os.makedirs(folder)
        _storage_save([gd], folder)
        d = torch.load(os.path.join(folder, "data.pth"), weights_only=True)
        assert np.array_equal(d["boards"].numpy().astype(np.uint8), npz[name + "__data_boards"])
        assert np.array_equal(d["values"].numpy(), npz[name + "__data_values"])
        assert np.array_equal(d["priors"].numpy(), npz[name + "__data_priors"])
        assert os.path.getsize(os.path.join(folder, "games.pkl")) > 0
        with open(os.path.join(folder, "games.pkl"), "rb") as f:
            back = pickle.load(f)
        assert [g.moves for g in back] == [gd.moves] and [g.result for g in back] == [gd.result]
        # the dataset reader's view of the file (Connect4Dataset.load, data.py:28-33): three tensors of one length
        assert len(d["boards"]) == len(d["values"]) == len(d["priors"]) == 2 * len(gd.moves)


def test_reference_result_count_works_on_mirror_results():
    RefResult = enum.Enum("Result", load_json("reference_result.json"))
    results = [gd.result for _, gd in _mirror_games()]
    counts = (results.count(RefResult.o_win), results.count(RefResult.draw), results.count(RefResult.x_win))
    assert sum(counts) == len(results) and sum(counts) > 0       # training.py:137-141 would print 0, 0, 0 otherwise
