"""The fused kernels libc4engine.so holds, one row per instantiation, and how to reach each of them.

c4_engine.hip compiles four families of fused kernels -- c4_selfplay_split_kernel<TS,MODE,TW,QUEUE>,
c4_selfplay_wave_kernel<TS,MODE,QUEUE>, c4_selfplay_kernel<TS,QUEUE> and c4_match_wave_kernel<TS,MODE> -- and
launch_split / launch_wave / launch_block / c4_match_steps choose among them at run time.  ROWS is the list of what is
compiled; `dispatch` is a model of that choice in plain Python.  tests/test_fused_matrix_host.py holds the two against
the built library (a new instantiation without a row here fails the CPU suite) and against each other (a row whose recipe
does not lead to its kernel fails there too); tests/test_gpu_fused_matrix.py launches every `verified` row, checks with
Engine.last_fused_kernel() that it was that kernel which ran, and compares its games / rows bit for bit with the
host-driven path (c4_step + c4_net_forward).

A NEW INSTANTIATION IS ENTERED HERE: its row, and a branch in `dispatch` if the launch functions gained one.

Row fields
  kernel   the name as c4_debug_last_fused_kernel spells it (without the run-time " spread=.. grid=.." tail)
  kind     "selfplay" (SelfPlay, fused_loop=True), "queue" (analysis.run_queue on a position-queue engine) or "match"
           (match.DeviceMatch)
  net      the net's mode: "f16" (32 filters, fp16 storage, MODE 0), "f32x3" (32 filters, reference precision, 1),
           "f16_64" (64 filters, fp16 storage, 2), "f32x3w" (64 filters, reference precision, 3); "f16" for the block kernel
  env      the values of C4_FUSED_MODE, C4_FUSED_SLOTS and C4_SPLIT_TW that lead there at a slot count that does not fill
           16 slots on every compute unit (any variable not named is unset)
  default  True when some caller reaches the kernel with no environment variable set (the 32-slot split kernels: with
           more than 16 slots per compute unit)
  status   "verified" (test_gpu_fused_matrix.py runs it) or "unverified: <reason>" -- never for a `default` row
"""
from collections import namedtuple

Row = namedtuple("Row", "kernel kind net env default status")

NET_MODES = {"f16": 0, "f32x3": 1, "f16_64": 2, "f32x3w": 3}
FAMILIES = ("c4_selfplay_split_kernel", "c4_selfplay_wave_kernel", "c4_selfplay_kernel", "c4_match_wave_kernel")
ENV_VARS = ("C4_FUSED_MODE", "C4_FUSED_SLOTS", "C4_SPLIT_TW")

# spelled by no launch function since launch_split chooses TW with `if constexpr`: a position-queue engine has the default
# split only (two tree waves for the 64-filter fp16 net, four for every other)
RETIRED = ("c4_selfplay_split_kernel<16,0,2,true>", "c4_selfplay_split_kernel<16,1,2,true>", "c4_selfplay_split_kernel<16,2,4,true>")


def E(**kw):
    """E(FUSED_MODE="wave", SPLIT_TW="3") -> {"C4_FUSED_MODE": "wave", "C4_SPLIT_TW": "3"}"""
    return {"C4_" + k: v for k, v in kw.items()}


R, V = Row, "verified"
ROWS = [
    # ---- tree waves + network waves, the default family.  C4_SPLIT_TW is read by self-play engines at 16 slots per workgroup
    # and not for f32x3w; a position-queue engine has the mode's default split only
    R("c4_selfplay_split_kernel<16,0,2,false>", "selfplay", "f16", E(SPLIT_TW="2"), False, V),
    R("c4_selfplay_split_kernel<16,0,3,false>", "selfplay", "f16", E(SPLIT_TW="3"), False, V),
    R("c4_selfplay_split_kernel<16,0,4,false>", "selfplay", "f16", E(), True, V),
    R("c4_selfplay_split_kernel<16,0,4,true>", "queue", "f16", E(), True, V),
    R("c4_selfplay_split_kernel<32,0,4,false>", "selfplay", "f16", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<32,0,4,true>", "queue", "f16", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<16,1,2,false>", "selfplay", "f32x3", E(SPLIT_TW="2"), False, V),
    R("c4_selfplay_split_kernel<16,1,3,false>", "selfplay", "f32x3", E(SPLIT_TW="3"), False, V),
    R("c4_selfplay_split_kernel<16,1,4,false>", "selfplay", "f32x3", E(), True, V),
    R("c4_selfplay_split_kernel<16,1,4,true>", "queue", "f32x3", E(), True, V),
    R("c4_selfplay_split_kernel<32,1,4,false>", "selfplay", "f32x3", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<32,1,4,true>", "queue", "f32x3", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<16,2,2,false>", "selfplay", "f16_64", E(), True, V),
    R("c4_selfplay_split_kernel<16,2,3,false>", "selfplay", "f16_64", E(SPLIT_TW="3"), False, V),
    R("c4_selfplay_split_kernel<16,2,4,false>", "selfplay", "f16_64", E(SPLIT_TW="4"), False, V),
    R("c4_selfplay_split_kernel<16,2,2,true>", "queue", "f16_64", E(), True, V),
    R("c4_selfplay_split_kernel<32,2,4,false>", "selfplay", "f16_64", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<32,2,4,true>", "queue", "f16_64", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<16,3,4,false>", "selfplay", "f32x3w", E(), True, V),
    R("c4_selfplay_split_kernel<16,3,4,true>", "queue", "f32x3w", E(), True, V),
    R("c4_selfplay_split_kernel<32,3,4,false>", "selfplay", "f32x3w", E(FUSED_SLOTS="32"), True, V),
    R("c4_selfplay_split_kernel<32,3,4,true>", "queue", "f32x3w", E(FUSED_SLOTS="32"), True, V),
    # ---- wave-autonomous (C4_FUSED_MODE=wave): every mode but f32x3w, whose planes do not fit a workgroup eight times
    R("c4_selfplay_wave_kernel<16,0,false>", "selfplay", "f16", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<16,0,true>", "queue", "f16", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<32,0,false>", "selfplay", "f16", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_wave_kernel<32,0,true>", "queue", "f16", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_wave_kernel<16,1,false>", "selfplay", "f32x3", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<16,1,true>", "queue", "f32x3", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<32,1,false>", "selfplay", "f32x3", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_wave_kernel<32,1,true>", "queue", "f32x3", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_wave_kernel<16,2,false>", "selfplay", "f16_64", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<16,2,true>", "queue", "f16_64", E(FUSED_MODE="wave"), False, V),
    R("c4_selfplay_wave_kernel<32,2,false>", "selfplay", "f16_64", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_wave_kernel<32,2,true>", "queue", "f16_64", E(FUSED_MODE="wave", FUSED_SLOTS="32"), False, V),
    # ---- workgroup-synchronous (C4_FUSED_MODE=block): the 32-filter fp16 net only
    R("c4_selfplay_kernel<16,false>", "selfplay", "f16", E(FUSED_MODE="block"), False, V),
    R("c4_selfplay_kernel<16,true>", "queue", "f16", E(FUSED_MODE="block"), False, V),
    R("c4_selfplay_kernel<32,false>", "selfplay", "f16", E(FUSED_MODE="block", FUSED_SLOTS="32"), False, V),
    R("c4_selfplay_kernel<32,true>", "queue", "f16", E(FUSED_MODE="block", FUSED_SLOTS="32"), False, V),
    # ---- net-vs-net matches: c4_match_steps reads none of the three variables
    R("c4_match_wave_kernel<16,0>", "match", "f16", E(), True, V),
    R("c4_match_wave_kernel<16,1>", "match", "f32x3", E(), True, V),
    R("c4_match_wave_kernel<16,2>", "match", "f16_64", E(), True, V),
]


def _b(queue):
    return "true" if queue else "false"


def atoi(s):
    """C's atoi on the value of an environment variable: leading blanks, a sign, digits; 0 when there are none."""
    s = s.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j] in "0123456789":
        j += 1
    return sign * int(s[i:j]) if j > i else 0


def launch_shape(kind, net, n_slots, env, cus=256, pack_dense=False):
    """What c4_engine_create and the launch functions make of (kind, net mode, slots, environment) on a device of `cus`
    compute units: (kernel name, spread, grid), as c4_debug_last_fused_kernel reports them.  ValueError where the engine
    refuses the combination (C4_ESTATE)."""
    mode = NET_MODES[net]
    if kind == "match":
        if net == "f32x3w":
            raise ValueError("c4_match_steps cannot hold the 64-filter reference-precision net")
        return "c4_match_wave_kernel<16,%d>" % mode, 0, (n_slots + 15) // 16
    if kind not in ("selfplay", "queue"):
        raise ValueError("kind is selfplay, queue or match")
    queue = kind == "queue"
    # c4_engine_create
    ts = 32 if n_slots > 16 * cus else 16
    fm = env.get("C4_FUSED_MODE")
    family = "split" if fm is None else {"block": "block", "wave": "wave"}.get(fm, "split")
    split_tw = atoi(env["C4_SPLIT_TW"]) if "C4_SPLIT_TW" in env else 0
    if "C4_FUSED_SLOTS" in env and atoi(env["C4_FUSED_SLOTS"]) in (16, 32):
        ts = atoi(env["C4_FUSED_SLOTS"])
    # c4_selfplay_steps
    if family == "block":
        if net != "f16":
            raise ValueError("C4_FUSED_MODE=block serves only the 32-filter fp16 net")
        return "c4_selfplay_kernel<%d,%s>" % (ts, _b(queue)), 0, (n_slots + ts - 1) // ts
    if family == "wave":
        if net == "f32x3w":
            raise ValueError("C4_FUSED_MODE=wave cannot hold the 64-filter reference-precision net")
        return "c4_selfplay_wave_kernel<%d,%d,%s>" % (ts, mode, _b(queue)), 0, (n_slots + ts - 1) // ts
    # launch_split
    dense_wgs = (n_slots + ts - 1) // ts
    spread = 1 if (not pack_dense and dense_wgs < cus and n_slots > dense_wgs) else 0
    grid = min(cus, n_slots) if spread else dense_wgs
    if ts == 32:
        tw = 4
    else:
        tw = 2 if net == "f16_64" else 4
        if not queue and net != "f32x3w" and split_tw:
            tw = split_tw if split_tw in (2, 3) else 4
    return "c4_selfplay_split_kernel<%d,%d,%d,%s>" % (ts, mode, tw, _b(queue)), spread, grid


def dispatch(kind, net, n_slots, env, cus=256):
    """The kernel name alone."""
    return launch_shape(kind, net, n_slots, env, cus)[0]


def reported(kind, net, n_slots, env, cus=256, pack_dense=False):
    """The whole string Engine.last_fused_kernel() must give after such a launch."""
    return "%s spread=%d grid=%d" % launch_shape(kind, net, n_slots, env, cus, pack_dense)
