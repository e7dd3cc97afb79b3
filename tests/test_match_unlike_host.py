"""Host side of device matches between unlike players (connect4_amd.match with unlike=True / kernel=..., c4_match_configure,
c4_match_split_kernel): the eligibility rules that are dropped and those that stay, the kernel choice, the instantiations
in the built library and the C prototype.  No GPU: the nets are FusedNet objects that were never handed to the device."""
import ctypes as C
import os
import re

import pytest

from connect4_amd import _lib as L
from connect4_amd import match as M
from connect4_amd.board import Board
from test_device_match_host import CASES, net_player

# what `unlike` drops, and what it keeps, among the refusals test_device_match_host.py pins
DROPPED = ("filters", "residual blocks", "precision", "f32x3w", "simulations", "pb_c_base", "pb_c_init")
KEPT = ("not an MCTS", "centre evaluator", "bare centre evaluator", "host callable", "not a FusedNet", "devices", "root noise", "sampling")


def test_every_pinned_refusal_is_either_dropped_or_kept():
    assert sorted(DROPPED + KEPT) == sorted(c[0] for c in CASES)


@pytest.mark.parametrize("name, make, reason", [c for c in CASES if c[0] in DROPPED], ids=[c[0] for c in CASES if c[0] in DROPPED])
def test_unlike_accepts_what_sameness_refused(name, make, reason):
    p1, p2 = make()
    assert reason in M.device_match_reason([p1, p2])                       # as the call is made today
    assert reason in M.device_match_reason([p1, p2], unlike=False)
    assert M.device_match_reason([p1, p2], unlike=True) is None
    assert M.device_match_reason([p1, p2, net_player("third", filters=64, precision="f32x3w")], unlike=True) is None
    m = M.DeviceMatch(False, p1, p2, plies=1, switch=True, unlike=True)
    assert m.unlike is True and m.kernel is None and len(m.games) == 14


@pytest.mark.parametrize("name, make, reason", [c for c in CASES if c[0] in KEPT], ids=[c[0] for c in CASES if c[0] in KEPT])
def test_unlike_keeps_the_other_rules(name, make, reason):
    p1, p2 = make()
    assert reason in M.device_match_reason([p1, p2], unlike=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.DeviceMatch(False, p1, p2, plies=1, switch=True, unlike=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.tournament([p1, p2], plies=1, switch=True, unlike=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.play_device_games([p1, p2], [(Board(), 0, 1)], unlike=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.play_device_games([p1, p2], [(Board(), 0, 1)], kernel="split")


def test_player_count_holds_for_unlike_matches():
    a = net_player("a")
    assert "2 to %d players" % L.MATCH_MAX_NETS in M.device_match_reason([a], unlike=True)
    assert "2 to %d players" % L.MATCH_MAX_NETS in M.device_match_reason([a] * (L.MATCH_MAX_NETS + 1), unlike=True)


def test_kernel_choice():
    wide = lambda n: net_player(n, filters=64, precision="f32x3w")  # noqa: E731
    nets = lambda *ps: [M._device_net(p) for p in ps]  # noqa: E731
    a, b, w = net_player("a"), net_player("b", precision="f16"), wide("w")
    assert M.match_kernels(nets(a, a)) is None                              # nothing to configure: the engine as it ever was
    assert M.match_kernels(nets(a, b, w), unlike=True) == ["wave", "wave", "split"]
    assert M.match_kernels(nets(a, b, w), unlike=True, kernel="split") == ["split"] * 3
    assert M.match_kernels(nets(a, a), kernel="split") == ["split", "split"]     # allowed between like players too
    assert M.match_kernels(nets(a, a), kernel="wave") == ["wave", "wave"]
    with pytest.raises(ValueError, match="f32x3w"):
        M.match_kernels(nets(a, w), unlike=True, kernel="wave")
    with pytest.raises(ValueError, match="kernel must be"):
        M.match_kernels(nets(a, a), kernel="block")
    # ... and through every entry point, before an engine exists
    for call in (lambda: M.DeviceMatch(False, wide("w1"), wide("w2"), plies=1, switch=True, unlike=True, kernel="wave"),
                 lambda: M.tournament([a, wide("w1")], plies=1, unlike=True, kernel="wave"),
                 lambda: M.play_device_games([a, wide("w1")], [(Board(), 0, 1)], unlike=True, kernel="wave"),
                 lambda: M.play_match(False, wide("w1"), wide("w2"), plies=1, unlike=True, kernel="wave")):
        with pytest.raises(ValueError, match="f32x3w"):
            call()
    # like players on the split kernel: the sameness rules still hold without `unlike`
    with pytest.raises(ValueError, match="f32x3w"):
        M.DeviceMatch(False, wide("w1"), wide("w2"), plies=1, kernel="split")
    assert M.DeviceMatch(False, a, net_player("a2"), plies=1, kernel="split").kernel == "split"


def test_new_keywords_are_handed_on_only_when_set(monkeypatch):
    seen = []

    def fake_play(players, games, n_steps, cache_bits, order, **kwargs):
        seen.append(kwargs)
        return [], {}
    monkeypatch.setattr(M, "play_device_games", fake_play)
    monkeypatch.setattr(M, "score_results", lambda *a: {"wins": 0, "draws": 0, "losses": 0, "return": 0.0})
    a, b = net_player("a"), net_player("b", filters=64, precision="f32x3w")
    M.DeviceMatch(False, a, net_player("a2"), plies=1).play()
    M.DeviceMatch(False, a, b, plies=1, unlike=True).play()
    M.DeviceMatch(False, a, b, plies=1, unlike=True, kernel="split", on_launch=len).play()
    assert seen == [{}, {"unlike": True}, {"on_launch": len, "unlike": True, "kernel": "split"}]
    assert M.play_match(False, a, b, plies=1, unlike=True) == ({"wins": 0, "draws": 0, "losses": 0, "return": 0.0}, "device")
    assert seen[-1] == {"unlike": True}


def test_play_match_goes_to_the_host_without_the_flag(monkeypatch):
    calls = []

    class Stub:
        def __init__(self, *args, **kwargs):
            calls.append((type(self).__name__, kwargs))

        def play(self, agents=1):
            return {}

    monkeypatch.setattr(M, "DeviceMatch", type("Device", (Stub,), {}))
    monkeypatch.setattr(M, "Match", type("Host", (Stub,), {}))
    a, b = net_player("a"), net_player("b", config=M_config(48))
    assert M.play_match(False, a, b, plies=1)[1] == "host"
    assert M.play_match(False, a, b, plies=1, unlike=True)[1] == "device"
    assert M.play_match(False, a, b, plies=1, unlike=True, kernel="split", n_steps=3)[1] == "device"
    assert calls == [("Host", {}), ("Device", {"unlike": True}), ("Device", {"unlike": True, "kernel": "split", "n_steps": 3})]


def M_config(sims):
    from connect4_amd.mcts import MCTSConfig
    return MCTSConfig(sims, pb_c_base=100, pb_c_init=2.0)


# ---------------------------------------------------------------- the library and the C ABI
SPLIT_MANGLED = re.compile(rb"c4_match_split_kernelILi(\d+)ELi(\d+)ELi(\d+)EE")


def test_library_holds_exactly_the_four_split_match_kernels():
    """One instantiation per net mode, with the tree waves launch_split picks at 16 slots for that mode (2 for the
    64-filter fp16 net, 4 otherwise)."""
    with open(L.LIB_PATH, "rb") as f:
        blob = f.read()
    names = {"c4_match_split_kernel<%d,%d,%d>" % tuple(int(x) for x in m.groups()) for m in SPLIT_MANGLED.finditer(blob)}
    assert names == {"c4_match_split_kernel<16,0,4>", "c4_match_split_kernel<16,1,4>", "c4_match_split_kernel<16,2,2>",
                     "c4_match_split_kernel<16,3,4>"}


def test_match_configure_is_declared_and_bound():
    with open(L.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+c4_match_configure\s*\(\s*c4_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*const\s+c4_match_player\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"#define\s+C4_MATCH_KERNEL_WAVE\s+0\b", text) and L.MATCH_KERNEL_WAVE == 0
    assert re.search(r"#define\s+C4_MATCH_KERNEL_SPLIT\s+1\b", text) and L.MATCH_KERNEL_SPLIT == 1
    assert re.search(r"#define\s+C4_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4      # an addition
    # the struct, field for field
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*c4_match_player\s*;", text)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t simulations", "int32_t pb_c_base", "double pb_c_init", "int32_t kernel", "int32_t reserved[3]"]
    assert [n for n, _ in L.MatchPlayer._fields_] == ["simulations", "pb_c_base", "pb_c_init", "kernel", "reserved"]
    assert C.sizeof(L.MatchPlayer) == 32 and L.MatchPlayer.pb_c_init.offset == 8 and L.MatchPlayer.kernel.offset == 16
    res, args = L.SIGNATURES["c4_match_configure"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.c_int32 and args[2] is C.POINTER(L.MatchPlayer)


def test_match_configure_refuses_a_null_engine():
    lib = L.load()
    p = L.MatchPlayer(simulations=32, pb_c_base=19652, pb_c_init=1.25, kernel=L.MATCH_KERNEL_SPLIT)
    assert lib.c4_match_configure(None, 0, C.byref(p)) == L.EINVAL


def test_engine_match_configure_checks_its_kernel_name():
    from connect4_amd.engine import Engine
    eng = object.__new__(Engine)       # no device behind it: the argument check comes first
    eng._h = None
    with pytest.raises(ValueError, match="'wave' or 'split'"):
        eng.match_configure(0, kernel="block")
    assert os.path.exists(L.LIB_PATH)
