"""CPU: the launch schedule of an engine (csrc/engine_schedule.cpp plan_schedule) on a container's tables alone -- include/adas_hip.h
adas_debug_engine_schedule, no device, no weight.

  recorded schedules  every shipped graph x 4 precisions x (max_batch, batch) = (64, 64), (64, 1), (1, 1), and the two 16-bit precisions
                      again with ADAS_ML=1, against tests/golden/engine_schedules.json.gz: every layer's adas_engine_layer_kernel string,
                      the launch count and adas_engine_ml_info, recorded from live engines on an MI355X with the engine as it was before
                      the schedule was decided in one place (make_golden_engine_schedules.py).  No exception: string for string.
  invariants          what step_of / role must satisfy on every one of those configurations
  boundaries          small hand-made graphs around the grouped launch and the folded shortcut; the expected schedules are written here
                      from the rules, not read back from the planner"""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_pkg

load_pkg()
L = importlib.import_module("adas_amd._lib")
M = importlib.import_module("adas_amd.models")
import make_golden_engine_schedules as G
import test_engine_plan_cpu as P          # the plan rows, the small-graph helpers and env()

F16, BF16, F32, X3 = L.PREC_FP16, L.PREC_BF16, L.PREC_FP32, L.PREC_FP16X3
Z = M.ZeroWeights()
# roles (include/adas_hip.h)
OWN, GROUP_LEAD, GROUP_MEMBER, ML_LEAD, ML_MEMBER, IN_SHORTCUT_USER, IN_CONSUMER_LOADS, IN_POOL3 = range(8)
C2F_LEAD, C2F_HIDDEN, C2F_TAIL, PAIR_FIRST, IN_PAIR, IN_DETECT, STEM_LEAD, STEM_INPUT, STEM_TAIL = range(8, 17)
LEADS = {OWN, GROUP_LEAD, ML_LEAD, C2F_LEAD, PAIR_FIRST, STEM_LEAD}
HIDDEN = {IN_SHORTCUT_USER, IN_CONSUMER_LOADS, C2F_LEAD, C2F_HIDDEN, PAIR_FIRST, IN_DETECT, STEM_LEAD, STEM_INPUT}     # no activation in memory
LABEL_CAP = 96
I32 = C.POINTER(C.c_int32)


def schedule(tables, prec, max_batch, batch):
    """(step_of, role, labels, n_steps) the engine decides for these table bytes at `batch` frames; AdasError where the loader refuses them."""
    n, ns = C.c_int32(), C.c_int32()
    L.check(L.lib().adas_debug_engine_schedule(tables, len(tables), prec, max_batch, batch, None, None, None, 0, C.byref(n), C.byref(ns)))
    step_of, role = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    lab = C.create_string_buffer(n.value * LABEL_CAP)
    L.check(L.lib().adas_debug_engine_schedule(tables, len(tables), prec, max_batch, batch, step_of.ctypes.data_as(I32), role.ctypes.data_as(I32), lab,
                                               n.value, C.byref(n), C.byref(ns)))
    labels = [lab.raw[i * LABEL_CAP:(i + 1) * LABEL_CAP].split(b"\0")[0].decode() for i in range(n.value)]
    return step_of, role, labels, ns.value


# -------------------------------------------------------------------------------------------------------------- recorded schedules
RECORDED = G.load()


def test_fixture_covers_every_shipped_configuration():
    assert set(RECORDED) == G.all_keys(M.BUILDERS)


def ml_items(g, rows, members, batch, prec):
    """The work items of one multi-layer launch over these layers, from the launch planner on layer descriptions (adas_debug_ml_plan)."""
    def view(v, c=None):
        h, w, cs, _ = g.bufs[v.buf]
        return L.MlView((v.buf + 1) << 12, cs, v.coff, v.c if c is None else c, h, w)
    descs = []
    for i in members:
        r, up = g.ops[i], int(rows[i, P.UP_SRC])
        descs.append(L.MlLayerDesc(int(rows[i, P.KERNEL]), r["stride"], r["act"], r["res_mode"], g.ops[up]["out"].c if up >= 0 else 0, int(rows[i, P.HALO_BN]),
                                   view(r["ins"][0]), view(r["out"]), view(r["res"], r["out"].c) if r["res"] else L.MlView(),
                                   view(g.ops[up]["ins"][0]) if up >= 0 else L.MlView()))
    n = len(descs)
    deps, tg, summ = (C.c_int32 * (6 * n))(), (C.c_int32 * (6 * n))(), (C.c_int32 * 4)()
    L.check(L.lib().adas_debug_ml_plan((L.MlLayerDesc * n)(*descs), n, batch, prec, deps, tg, None, 0, summ))
    return summ[0]


def check_invariants(key, rows, step_of, role, labels, n_steps, grouped):
    n = len(role)
    assert ((step_of >= -1) & (step_of < n_steps)).all(), key
    # nothing computes exactly the layers folded into their consumer's loads; they are skipped in the plan, and so is every layer that
    # rides in a fused launch of the plan's
    assert ((step_of == -1) == (role == IN_CONSUMER_LOADS)).all(), key
    riders = np.isin(role, [IN_CONSUMER_LOADS, IN_POOL3, C2F_HIDDEN, C2F_TAIL, IN_PAIR, IN_DETECT, STEM_INPUT, STEM_TAIL])
    assert (riders == (rows[:, P.SKIP] == 1)).all(), key
    lead_of = np.full(n_steps, -1)
    for l in range(n):
        if role[l] in LEADS:
            assert lead_of[step_of[l]] == -1, (key, "two leads in step", int(step_of[l]))      # each step has one lead ...
            lead_of[step_of[l]] = l
        elif step_of[l] >= 0:
            assert labels[l].startswith(("(in ", "(fused ")), (key, l, labels[l])
        else:
            assert labels[l] == "(folded into the consumer's loads)", (key, l, labels[l])
    assert (lead_of >= 0).all(), key                                                            # ... and every step one
    for l in range(n):                                # a shared launch's lead is its first layer
        if role[l] in (GROUP_MEMBER, ML_MEMBER):
            assert lead_of[step_of[l]] < l and role[lead_of[step_of[l]]] == role[l] - 1, (key, l)
    # launch order is layer order, except inside a grouped run (level by level): only its 3x3 convs may be out of order
    for k in np.flatnonzero(np.diff(lead_of) < 0):
        assert grouped and {int(role[lead_of[k]]), int(role[lead_of[k + 1]])} <= {OWN, GROUP_LEAD}, (key, int(k))
        assert rows[lead_of[k], P.KERNEL] == rows[lead_of[k + 1], P.KERNEL] == 1, (key, int(k))                   # CONV_HALO
    if not grouped:
        assert not np.isin(role, [GROUP_LEAD, GROUP_MEMBER]).any(), key


@pytest.mark.parametrize("name", list(M.BUILDERS))
def test_recorded_schedule(name):
    g = M.build(name, wsrc=Z)
    tables = g.tables()
    for ml in (False, True):
        for prec in (G.ML_PRECISIONS if ml else G.PRECISIONS):
            for mb, b in G.SHAPES:
                key = G.config_key(name, prec, mb, b, ml)
                want = RECORDED[key]
                with P.env(**({"ADAS_ML": "1"} if ml else {})):
                    if isinstance(want, str):
                        with pytest.raises(L.AdasError) as ex:
                            schedule(tables, L.PRECISIONS[prec], mb, b)
                        assert ex.value.code == -3 and G.refusal_text(str(ex.value)) == want, key
                        continue
                    step_of, role, labels, n_steps = schedule(tables, L.PRECISIONS[prec], mb, b)
                assert len(labels) == len(want["labels"]), key
                bad = [(i, a, w) for i, (a, w) in enumerate(zip(labels, want["labels"])) if a != w]
                assert not bad, (key, "first differing (layer, got, recorded):", bad[0])
                assert n_steps == want["launches"], key
                rows, _ = P.plan(tables, L.PRECISIONS[prec], mb)
                check_invariants(key, rows, step_of, role, labels, n_steps, grouped=not ml and prec in G.ML_PRECISIONS)
                if ml:
                    leads = [l for l in range(len(role)) if role[l] == ML_LEAD]
                    members = [[l] + [m for m in range(len(role)) if role[m] == ML_MEMBER and step_of[m] == step_of[l]] for l in leads]
                    items = sum(ml_items(g, rows, m, b, L.PRECISIONS[prec]) for m in members)
                    assert (len(leads), sum(len(m) for m in members), items) == want["ml"], key
                    for l, m in zip(leads, members):
                        assert labels[l] == f"conv_ml_kernel[{len(m)} layers]", key
                else:
                    assert not np.isin(role, [ML_LEAD, ML_MEMBER]).any(), key


# --------------------------------------------------------------------------------------------------------------------- boundaries
H, W = P.H, P.W
RELU = M.ACT_RELU          # (ReLU: never the first conv of a 3x3 pair)


def sched(g, prec, max_batch=2, batch=2):
    return schedule(g.tables(), prec, max_batch, batch)


def fan_graph(n, chain=False, pool_after=None):
    """n 3x3 convs "k0".."k<n-1>" on one 32-channel map (chain: each reads the one before); pool_after: a max-pool behind that many."""
    g, x0 = P.body(32)
    x = x0
    for i in range(n):
        if pool_after == i:
            g.maxpool(x0, 3, 1, 1, name="mp")
        y = g.conv(x, 32, 3, 1, f"k{i}", act=RELU)
        x = y if chain else x0
    return g


def ids(g, n):
    return [P.idx(g, f"k{i}") for i in range(n)]


@pytest.mark.parametrize("prec", [F16, BF16], ids=["fp16", "bf16"])
def test_two_independent_convs_share_a_launch(prec):
    g = fan_graph(2)
    a, b = ids(g, 2)
    step_of, role, labels, n_steps = sched(g, prec)
    assert (role[a], role[b]) == (GROUP_LEAD, GROUP_MEMBER) and step_of[a] == step_of[b]
    assert labels[a] == "conv_halo_group_kernel[2 layers]" and labels[b] == "(in the grouped launch)"
    assert n_steps == len(g.ops) - 1 and np.count_nonzero(step_of == step_of[a]) == 2       # input, c0, {k0, k1}


def test_a_chain_of_two_does_not_group():
    g = fan_graph(2, chain=True)
    a, b = ids(g, 2)
    step_of, role, labels, n_steps = sched(g, F16)
    assert (role == OWN).all() and step_of.tolist() == list(range(len(g.ops))) and n_steps == len(g.ops)
    assert labels[a].startswith("conv_") and labels[b].startswith("conv_") and "group" not in labels[a] + labels[b]


def test_nine_independent_convs_split_8_and_1():
    g = fan_graph(9)
    k = ids(g, 9)
    step_of, role, labels, n_steps = sched(g, F16)
    assert role[k].tolist() == [GROUP_LEAD] + [GROUP_MEMBER] * 7 + [OWN]
    assert len(set(step_of[k[:8]])) == 1 and step_of[k[8]] == step_of[k[0]] + 1
    assert labels[k[0]] == "conv_halo_group_kernel[8 layers]" and "group" not in labels[k[8]]
    assert n_steps == len(g.ops) - 7


def test_a_max_pool_breaks_the_run():
    g = fan_graph(4, pool_after=2)
    k, mp = ids(g, 4), P.idx(g, "mp")
    step_of, role, labels, n_steps = sched(g, F16)
    assert role[k].tolist() == [GROUP_LEAD, GROUP_MEMBER, GROUP_LEAD, GROUP_MEMBER] and role[mp] == OWN
    assert step_of[k[0]] == step_of[k[1]] < step_of[mp] < step_of[k[2]] == step_of[k[3]]
    assert labels[k[0]] == labels[k[2]] == "conv_halo_group_kernel[2 layers]" and labels[mp] == "maxpool_kernel"
    assert n_steps == len(g.ops) - 2


@pytest.mark.parametrize("prec", [F32, X3], ids=["fp32", "fp16x3"])
def test_only_the_16_bit_precisions_group(prec):
    g = fan_graph(9)
    step_of, role, labels, n_steps = sched(g, prec)
    assert (role == OWN).all() and step_of.tolist() == list(range(len(g.ops))) and n_steps == len(g.ops)


def test_no_group_switch_gives_the_plain_schedule():
    g = fan_graph(9)
    with P.env(ADAS_NO_GROUP="1"):
        step_of, role, labels, n_steps = sched(g, F16)
    assert (role == OWN).all() and step_of.tolist() == list(range(len(g.ops))) and n_steps == len(g.ops)
    assert GROUP_LEAD in sched(g, F16)[1]


def resnet_block(wsrc=Z):
    """ResNet layer2.0 (tests/test_gpu_conv.py test_projection_shortcut_folded_into_conv2): out = relu(conv3x3(t) + conv1x1_s2(x))."""
    g = M.Graph("t", 3, 80, 400, wsrc)
    x0, c3 = g.input()
    x = g.conv(x0, 64, 1, 1, "expand", act=RELU, true_cin=c3)
    t = g.conv(x, 128, 3, 2, "conv1", act=RELU)
    d = g.conv(x, 128, 1, 2, "down", act=M.ACT_NONE, pad=0)
    g.conv(t, 128, 3, 1, "conv2", act=RELU, res=d, res_mode=M.RES_BEFORE_ACT)
    return g


@pytest.mark.parametrize("prec", [F16, BF16], ids=["fp16", "bf16"])
def test_projection_shortcut_folds_by_batch(prec):
    """The link is the plan's; whether conv2's launch takes the projection is the schedule's, per batch: at 64 frames conv_h8 runs conv2
    and carries it, at one frame it cannot, and the projection launches on its own."""
    g = resnet_block()
    d, c2 = P.idx(g, "down"), P.idx(g, "conv2")
    rows, _ = P.plan(g.tables(), prec, 64)
    assert rows[c2, P.DS_SRC] == d and not rows[:, P.SKIP].any()
    step_of, role, labels, n_steps = sched(g, prec, 64, 64)
    assert role[d] == IN_SHORTCUT_USER and role[c2] == OWN and step_of[d] == step_of[c2] and n_steps == len(g.ops) - 1
    assert labels[d] == "(fused into the conv it is the shortcut of)" and labels[c2].startswith("conv_h8_kernel") and labels[c2].endswith("+shortcut")
    step_of, role, labels, n_steps = sched(g, prec, 64, 1)
    assert (role == OWN).all() and step_of.tolist() == list(range(len(g.ops))) and n_steps == len(g.ops)
    assert labels[d].startswith("conv_pw_kernel") and "+shortcut" not in labels[c2]


def test_hidden_roles_on_yolov8n():
    """Stem, C2f, SPPF, upsample fold and Detect roles all occur in YOLOv8n at fp16 (tests/test_gpu_engine_schedule.py refuses to fetch
    exactly the hidden ones)."""
    g = M.build("yolov8n", wsrc=Z)
    step_of, role, labels, n_steps = sched(g, F16, 64, 64)
    for r in (STEM_LEAD, STEM_INPUT, STEM_TAIL, C2F_LEAD, C2F_HIDDEN, C2F_TAIL, IN_POOL3, IN_CONSUMER_LOADS, IN_DETECT, PAIR_FIRST, IN_PAIR, GROUP_LEAD):
        assert r in role, r
    i = P.idx(g, "model.2.cv1.conv")
    assert role[i] == C2F_LEAD and [int(role[P.idx(g, "model.2." + n)]) for n in ("m.0.cv1.conv", "m.0.cv2.conv", "cv2.conv")] == [C2F_HIDDEN, C2F_HIDDEN, C2F_TAIL]
    assert role[0] == STEM_INPUT and role[1] == STEM_LEAD and role[2] == STEM_TAIL and step_of[0] == step_of[1] == step_of[2] == 0
