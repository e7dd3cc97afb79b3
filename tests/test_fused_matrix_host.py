"""tests/fused_matrix.py against the built library and against itself; no GPU.

hipcc registers every kernel with the HIP runtime under its mangled name, so libc4engine.so holds the names of the fused
kernels it was compiled with as plain strings, template arguments included.  The set found there must be the set of rows
of the matrix: an instantiation added to a launch function without a row -- and so without a GPU case that launches it and
compares what it plays -- fails here, as does a row whose kernel is gone.  The rows' recipes are checked against a Python
model of the dispatcher, so a wrong recipe is found before a GPU is needed (on the GPU the engine's own record of the
launch, c4_debug_last_fused_kernel, is compared with the same names)."""
import ctypes as C
import re

import pytest

import fused_matrix as fm

MANGLED = re.compile(rb"c4_(selfplay_split|selfplay_wave|selfplay|match_wave)_kernelI((?:Li\d+E|Lb[01]E)+)E")
ARG = re.compile(rb"Li(\d+)E|Lb([01])E")
SPELLING = re.compile(r"^(c4_selfplay_split_kernel<(16|32),[0-3],[234],(true|false)>|c4_selfplay_wave_kernel<(16|32),[0-2],(true|false)>|"
                      r"c4_selfplay_kernel<(16|32),(true|false)>|c4_match_wave_kernel<16,[0-2]>)$")


def demangle(family, args):
    """(b"selfplay_split", b"Li16ELi1ELi3ELb0E") -> "c4_selfplay_split_kernel<16,1,3,false>" """
    out = []
    for m in ARG.finditer(args):
        out.append(m.group(1).decode() if m.group(1) is not None else ("true" if m.group(2) == b"1" else "false"))
    return "c4_%s_kernel<%s>" % (family.decode(), ",".join(out))


@pytest.fixture(scope="module")
def compiled():
    import __graft_entry__ as g
    with open(g.build_engine(), "rb") as f:
        blob = f.read()
    return {demangle(*m.groups()) for m in MANGLED.finditer(blob)}


def test_demangle():
    m = MANGLED.search(b"_ZN12_GLOBAL__N_124c4_selfplay_split_kernelILi16ELi1ELi3ELb0EEEvPKNS_3DevEN5c4net6NetDevEPfS6_ii")
    assert demangle(*m.groups()) == "c4_selfplay_split_kernel<16,1,3,false>"
    m = MANGLED.search(b"_ZN12_GLOBAL__N_118c4_selfplay_kernelILi32ELb1EEEvNS_3DevEN5c4net6NetDevEPfS4_i")
    assert demangle(*m.groups()) == "c4_selfplay_kernel<32,true>"
    m = MANGLED.search(b"_ZN12_GLOBAL__N_120c4_match_wave_kernelILi16ELi2EEEvPKNS_3DevE")
    assert demangle(*m.groups()) == "c4_match_wave_kernel<16,2>"
    assert MANGLED.search(b"_ZN12_GLOBAL__N_114c4_step_kernelILi0ELb0EEEvNS_3DevEPKvS3_Pv") is None


def test_the_table_is_well_formed():
    names = [r.kernel for r in fm.ROWS]
    assert len(set(names)) == len(names), "a kernel has two rows"
    per_family = {f: sum(n.startswith(f + "<") for n in names) for f in fm.FAMILIES}
    assert per_family == {"c4_selfplay_split_kernel": 22, "c4_selfplay_wave_kernel": 12, "c4_selfplay_kernel": 4, "c4_match_wave_kernel": 3}
    for r in fm.ROWS:
        assert SPELLING.match(r.kernel), r.kernel
        assert r.kind in ("selfplay", "queue", "match") and r.net in fm.NET_MODES
        assert set(r.env) <= set(fm.ENV_VARS) and all(isinstance(v, str) for v in r.env.values())
        assert r.default in (True, False)
        assert r.status == "verified" or re.match(r"unverified: \S", r.status), r
        # the name's QUEUE and MODE arguments are the row's kind and net
        if r.kind != "match":
            assert r.kernel.endswith(",true>") == (r.kind == "queue"), r
        if not r.kernel.startswith("c4_selfplay_kernel<"):
            assert int(r.kernel.split("<")[1].split(",")[1].rstrip(">")) == fm.NET_MODES[r.net], r


def test_compiled_equals_the_table(compiled):
    rows = {r.kernel for r in fm.ROWS}
    assert compiled - rows == set(), "compiled into libc4engine.so without a row in tests/fused_matrix.py"
    assert rows - compiled == set(), "rows of tests/fused_matrix.py that libc4engine.so does not hold"
    assert len(compiled) == 41


def test_retired_instantiations_are_gone(compiled):
    assert len(fm.RETIRED) == 3
    for name in fm.RETIRED:
        assert SPELLING.match(name) and name not in compiled, name
        assert name not in {r.kernel for r in fm.ROWS}


def test_every_default_kernel_is_verified():
    for r in fm.ROWS:
        if r.default:
            assert r.status == "verified", "%s is reached with no environment variable set and has no GPU case: %s" % (r.kernel, r.status)
    # what no variable leads to, by the model: the default split at 16 and (beyond 16 slots per compute unit) at 32 slots
    # per workgroup, queue or not, and the match kernels
    reach = set()
    for net in fm.NET_MODES:
        for kind in ("selfplay", "queue", "match"):
            for n_slots in (35, 16 * 256 + 1):
                try:
                    reach.add(fm.dispatch(kind, net, n_slots, {}))
                except ValueError:
                    assert (kind, net) == ("match", "f32x3w")
    assert reach == {r.kernel for r in fm.ROWS if r.default}


@pytest.mark.parametrize("n_slots", [35, 14, 1, 4096])
def test_every_recipe_leads_to_its_kernel(n_slots):
    for r in fm.ROWS:
        assert fm.dispatch(r.kind, r.net, n_slots, r.env) == r.kernel, r


def test_the_model_reaches_nothing_but_the_table():
    """Every combination of the variables' values the engine tells apart, every net, kind and both sides of the
    16-slots-per-compute-unit threshold: a table row or a refusal, and every row is reached."""
    rows = {r.kernel for r in fm.ROWS}
    seen = set()
    for mode in (None, "split", "wave", "block", "junk"):
        for slots in (None, "16", "32", "8", "64", ""):
            for tw in (None, "2", "3", "4", "0", "5", "-1", "x"):
                env = {k: v for k, v in zip(fm.ENV_VARS, (mode, slots, tw)) if v is not None}
                for net in fm.NET_MODES:
                    for kind in ("selfplay", "queue", "match"):
                        for n_slots in (35, 16 * 256 + 1):
                            try:
                                name = fm.dispatch(kind, net, n_slots, env)
                            except ValueError:
                                continue
                            assert name in rows, (name, kind, net, n_slots, env)
                            seen.add(name)
    assert seen == rows


def test_ignored_variables_lead_to_the_default_kernel():
    """What issue a test must not fall for: a variable the dispatcher ignores leaves the default kernel running."""
    assert fm.dispatch("queue", "f32x3", 35, {"C4_SPLIT_TW": "2"}) == "c4_selfplay_split_kernel<16,1,4,true>"
    assert fm.dispatch("queue", "f16_64", 35, {"C4_SPLIT_TW": "4"}) == "c4_selfplay_split_kernel<16,2,2,true>"
    assert fm.dispatch("selfplay", "f32x3w", 35, {"C4_SPLIT_TW": "2"}) == "c4_selfplay_split_kernel<16,3,4,false>"
    assert fm.dispatch("selfplay", "f16", 35, {"C4_FUSED_SLOTS": "24"}) == "c4_selfplay_split_kernel<16,0,4,false>"
    assert fm.dispatch("selfplay", "f16", 35, {"C4_FUSED_SLOTS": "32", "C4_SPLIT_TW": "2"}) == "c4_selfplay_split_kernel<32,0,4,false>"
    assert fm.dispatch("match", "f16", 14, {"C4_FUSED_MODE": "block", "C4_FUSED_SLOTS": "32"}) == "c4_match_wave_kernel<16,0>"


def test_launch_shapes():
    """35 slots, dense: two full workgroups of 16 and one of 3, or one of 32 and one of 3; spread: one slot or two per
    workgroup; the wave, block and match kernels never spread."""
    assert fm.reported("selfplay", "f32x3", 35, {"C4_SPLIT_TW": "3"}, pack_dense=True) == "c4_selfplay_split_kernel<16,1,3,false> spread=0 grid=3"
    assert fm.reported("selfplay", "f32x3", 35, {"C4_FUSED_SLOTS": "32"}, pack_dense=True) == "c4_selfplay_split_kernel<32,1,4,false> spread=0 grid=2"
    assert fm.reported("selfplay", "f32x3", 35, {}) == "c4_selfplay_split_kernel<16,1,4,false> spread=1 grid=35"
    assert fm.reported("selfplay", "f16_64", 288, {}, cus=256) == "c4_selfplay_split_kernel<16,2,2,false> spread=1 grid=256"
    assert fm.reported("selfplay", "f16_64", 288, {}, cus=256, pack_dense=True) == "c4_selfplay_split_kernel<16,2,2,false> spread=0 grid=18"
    assert fm.reported("selfplay", "f16", 1, {}) == "c4_selfplay_split_kernel<16,0,4,false> spread=0 grid=1"
    assert fm.reported("queue", "f16", 35, {"C4_FUSED_MODE": "wave"}) == "c4_selfplay_wave_kernel<16,0,true> spread=0 grid=3"
    assert fm.reported("queue", "f16", 35, {"C4_FUSED_MODE": "block", "C4_FUSED_SLOTS": "32"}) == "c4_selfplay_kernel<32,true> spread=0 grid=2"
    assert fm.reported("match", "f16_64", 14, {}) == "c4_match_wave_kernel<16,2> spread=0 grid=1"


def test_atoi():
    assert [fm.atoi(s) for s in ("32", " 16", "3x", "x3", "", "-2", "+4", "016")] == [32, 16, 3, 0, 0, -2, 4, 16]


def test_the_entry_point_is_declared_bound_and_refuses_null():
    from connect4_amd import _lib as L
    with open(L.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+c4_debug_last_fused_kernel\s*\(\s*c4_engine\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    res, args = L.SIGNATURES["c4_debug_last_fused_kernel"]
    assert res is C.c_int and args == [C.c_void_p, C.c_char_p, C.c_int]
    assert re.search(r"#define\s+C4_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4      # an addition
    lib = L.load()
    buf = C.create_string_buffer(b"untouched", 64)
    assert lib.c4_debug_last_fused_kernel(None, buf, 64) == L.EINVAL and buf.value == b"untouched"
    from connect4_amd.engine import Engine
    assert callable(Engine.last_fused_kernel)
