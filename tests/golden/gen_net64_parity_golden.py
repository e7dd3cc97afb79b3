#!/usr/bin/env python3
"""Generate tests/golden/net64_parity.json and net64_parity_tables.npz: the reference's own 800-simulation searches with a
net of its example configuration (data/example_config.py: 64 filters, 6 residual blocks, 6 value-head Linear layers), and
for each of them whether the reference DECIDES it by a margin or whether it is a near-tie -- the recipe of
gen_net_parity_golden.py (whose helpers this imports) for the 64-filter reference-precision forward ("f32x3w").

It imports the UNMODIFIED reference over oracle/refshim and runs in the build container only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 \
      PYTHONPATH=<repo>/oracle/refshim:<reference> python <repo>/tests/golden/gen_net64_parity_golden.py

Everything written is data; a re-run reproduces both files byte for byte.

Net: the reference's ModelWrapper(ModelConfig(net_config=NetConfig(filters=64, n_fc_layers=6, n_residuals=6),
use_gpu=False)) with tests/net_models.stressed_state_dict(NetConfig(filters=64, n_residuals=6, n_fc_layers=6), seed=26)
loaded into its .net (the keys load as they are).  The weights come from numpy.random.RandomState and are not stored:
`weights_sha256` is the SHA-256 of their float32 bytes, keys in sorted order (num_batches_tracked left out).

Cases (recorded exactly as in net_parity.json):
  family A  24 seeded random undecided positions, ages spread over 0..33, mcts.search with 800 simulations, no noise;
  family B  every ply of one training_game() (800 simulations, alpha 0.3, fraction 0.25, 6 sampling moves; np.random.seed 0).

`decided` / `self_tv`: as gen_net_parity_golden.judge, K = 6, EPS = 16 x 15 x 2^-22 = tests/net_models.tol_f32x3(6).
Cap (a condition, not a tolerance): at least half of each family must be decided; asserted below.

Tables: the evaluator's position_table of the first eight A cases and of every fourth ply; if a written file would pass
1 MB, the table cases are thinned from the end (whole tables only) until it does not.
"""
import hashlib
import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, REPO)
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import gen_net_parity_golden as G  # noqa: E402
from gen_golden import GammaRecorder, random_position  # noqa: E402
from oinkoink.mcts import MCTSConfig  # noqa: E402
from oinkoink.neural.config import ModelConfig, NetConfig  # noqa: E402
from oinkoink.neural.pytorch.model import ModelWrapper  # noqa: E402
from oinkoink.neural.training_game import training_game  # noqa: E402
from oracle import c4oracle as oc  # noqa: E402

import net_models  # noqa: E402
from connect4_amd.net import NetConfig as PkgNetConfig  # noqa: E402

FILTERS, RESIDUALS, FC_LAYERS, NET_SEED = 64, 6, 6, 26
EPS = 16 * (2 * RESIDUALS + 3) * 2.0 ** -22     # tests/net_models.tol_f32x3(6); test_net64_fixture.py checks the two agree
K = 6
N_A, AGE_MAX, N_A_TABLES = 24, 33, 8
GAME_SEED = 0
SIMS = 800
MAX_BYTES = 1000000
G.EPS, G.K = EPS, K      # the imported perturbation() and judge() read their module's constants


def weights_sha256(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        if not k.endswith("num_batches_tracked"):
            h.update(np.ascontiguousarray(sd[k].numpy().astype(np.float32)).tobytes())
    return h.hexdigest()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)  # deterministic accumulation order for the recorded net outputs
    oc.build()
    sd = net_models.stressed_state_dict(PkgNetConfig(filters=FILTERS, n_residuals=RESIDUALS, n_fc_layers=FC_LAYERS), seed=NET_SEED)
    wrapper = ModelWrapper(ModelConfig(net_config=NetConfig(filters=FILTERS, n_fc_layers=FC_LAYERS, n_residuals=RESIDUALS), use_gpu=False))
    wrapper.net.load_state_dict(sd, strict=True)
    memo = G.MemoModel(wrapper)
    cases, tables = [], {}

    rng = np.random.RandomState(2064)
    seen = set()
    for i in range(N_A):
        age = int(round(i * AGE_MAX / (N_A - 1.0)))
        while True:
            b = random_position(rng, age)
            if (int(b.color[0]), int(b.color[1])) not in seen:
                break
        seen.add((int(b.color[0]), int(b.color[1])))
        cases.append(G.searched("A%02d_s%d" % (i, SIMS), "A", b, MCTSConfig(SIMS), memo, tables, i < N_A_TABLES))
        print(cases[-1]["name"], "age", age, cases[-1]["N"], flush=True)

    cfg = MCTSConfig(SIMS, root_dirichlet_alpha=0.3, root_exploration_fraction=0.25, num_sampling_moves=6)
    np.random.seed(GAME_SEED)
    with GammaRecorder() as rec:
        player = G.RecordingMCTS("ref", cfg, memo, rec, GAME_SEED, tables)
        gd = training_game(player)
    assert len(player.cases) == len(gd.moves)
    for d, mv, pol, v in zip(player.cases, gd.moves, gd.priors, gd.values):
        assert d["move"] == int(mv) and d["value"] == (None if v is None else float(v))
        d["policy"] = [float(x) for x in pol]
        assert d["policy"] == d["values_policy"]
    cases.extend(player.cases)
    games = [dict(seed=GAME_SEED, moves=[int(m) for m in gd.moves], result=float(gd.result.value))]
    print("game", GAME_SEED, games[-1]["moves"], flush=True)

    for c in cases:
        G.judge(c, memo)
        print(c["name"], "decided" if c["decided"] else "near-tie", "self_tv %.4f" % c["self_tv"], flush=True)
    share = {f: float(np.mean([c["decided"] for c in cases if c["family"] == f])) for f in ("A", "B")}
    print("decided shares:", share)
    assert share["A"] >= 0.5 and share["B"] >= 0.5, share

    npz_path, json_path = os.path.join(OUT, "net64_parity_tables.npz"), os.path.join(OUT, "net64_parity.json")
    kept = [c["name"] for c in cases if c["name"] in tables]
    while True:
        blobs = {}
        for name in kept:
            for k, a in zip(("c0", "c1", "v", "p"), tables[name]):
                blobs["%s__%s" % (name, k)] = a
        G.write_npz(npz_path, blobs)
        if os.path.getsize(npz_path) <= MAX_BYTES:
            break
        kept.pop()      # whole tables only, from the end
    with_table = [c for c in cases if c["name"] in kept]
    assert any(c["decided"] for c in with_table) and any(not c["decided"] for c in with_table)
    with open(json_path, "w") as f:
        json.dump(dict(eps=EPS, K=K, decided_share=share, table_cases=kept, games=games, weights_sha256=weights_sha256(sd),
                       net=dict(filters=FILTERS, n_residuals=RESIDUALS, n_fc_layers=FC_LAYERS, seed=NET_SEED), cases=cases), f)
    assert os.path.getsize(json_path) <= MAX_BYTES
    print("%d cases, %d tables, %d table positions written to %s" % (len(cases), len(kept), sum(len(tables[n][0]) for n in kept), OUT))


if __name__ == "__main__":
    main()
