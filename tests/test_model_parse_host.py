"""
The host side of lm_model_create without a device: csrc/lm_model_parse.h (every check of an untrusted chain-model blob, the derived task
facts) and csrc/lm_families.h (which kernel family serves a model, which kernel kinds a family has), run under the address and
undefined-behaviour sanitizers as a stand-alone program (tests/model_parse_main.cpp) over the lowering of every shipped model.
"""

import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import test_plain_layout_gpu as G
from loco_mujoco_amd import lowering, mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "loco_mujoco_amd", "assets")
MESH = os.path.join(ROOT, "tests", "golden", "humanoid_torque_mesh_feet.model.npz")

# The kernel family of every shipped model (loco_mujoco_amd/assets/<name>.model.npz, lowered with the neutral task below), and of four
# more blobs so that every family occurs: the mesh-foot fixture (seven-link chains), the muscle humanoid lowered without its pair
# tables, and two shipped models with the header's integrator set to RK4 — a quadruped nothing is specialised for (generic kernels)
# and six-link chains no kernel is compiled for (-1). Recorded from the selection rule as it stood in lm_kernels.hip (family_of) before
# it moved into lm_families.h: that rule, copied verbatim into a scratch program, run over these same blobs.
FAMILIES = {
    "Atlas.back": 2, "Atlas.carry.default.w0.1": 2, "Atlas.carry.default.w1": 2, "Atlas.carry.default.w10": 2, "Atlas.carry.default.w5": 2,
    "Atlas.default": 2, "HumanoidMuscle.default": 10, "HumanoidMuscle.s0.4": 10, "HumanoidMuscle.s0.6": 10, "HumanoidMuscle.s0.8": 10,
    "HumanoidMuscle.s1": 10, "HumanoidTorque.default": 8, "HumanoidTorque.s0.4": 8, "HumanoidTorque.s0.6": 8, "HumanoidTorque.s0.8": 8,
    "HumanoidTorque.s1": 8, "Talos.carry.default.w0.1": 4, "Talos.carry.default.w1": 4, "Talos.carry.default.w10": 4,
    "Talos.carry.default.w5": 4, "Talos.default": 4, "Talos.noback": 4, "UnitreeA1.position": 0, "UnitreeA1.torque": 0,
    "UnitreeG1.default": 7, "UnitreeG1.legs": 7, "UnitreeG1.noarms": 7, "UnitreeG1.noback": 7, "UnitreeH1.arms": 7,
    "UnitreeH1.carry.default.w0.1": 9, "UnitreeH1.carry.default.w1": 9, "UnitreeH1.carry.default.w10": 9, "UnitreeH1.carry.default.w5": 9,
    "UnitreeH1.default": 9, "UnitreeH1.noback": 9,
}
EXTRA = {"mesh_feet": 11, "HumanoidMuscle.default.nopairs": 5, "UnitreeA1.torque.rk4": 6, "UnitreeG1.legs.rk4": -1}
# The models of tests/test_generic_family_gpu.py (generic_family_common.CASES: the compiled model edited before it is lowered), so that
# none of them drifts into a specialised family unnoticed; and the two such edits that have no kernel: six-link chains under an elliptic
# cone, and a muscle model under one — the generic kernels are compiled without muscles, so pick_family refuses it.
EDITED = {"UnitreeA1.torque.pyramidal3": ("UnitreeA1.torque", "_pyramidal_condim3", 6), "Talos.default.elliptic": ("Talos.default", "_elliptic", 6),
          "Atlas.default.elliptic": ("Atlas.default", "_elliptic", 6), "HumanoidTorque.default.elliptic": ("HumanoidTorque.default", "_elliptic", 6),
          "UnitreeH1.default.elliptic": ("UnitreeH1.default", "_elliptic", 6), "UnitreeG1.default.elliptic": ("UnitreeG1.default", "_elliptic", -1),
          "HumanoidMuscle.default.elliptic": ("HumanoidMuscle.default", "_elliptic", -1)}
EXTRA.update((k, v[2]) for k, v in EDITED.items())
# the instance <links, slots, RK4> of the generic family that serves each of its blobs (lm_families.h generic_instance)
GENERIC_INSTANCE = {"UnitreeA1.torque.rk4": (3, 4, 1), "UnitreeA1.torque.pyramidal3": (3, 4, 0), "Talos.default.elliptic": (5, 8, 0), "Atlas.default.elliptic": (5, 8, 1),
                    "HumanoidTorque.default.elliptic": (5, 8, 1), "UnitreeH1.default.elliptic": (5, 8, 0)}
# the tasks of tests/test_plain_layout_gpu.py FAMILY and the blob of the same robot here
SAME_ROBOT = {"UnitreeA1.simple": "UnitreeA1.torque", "Atlas.walk": "Atlas.default", "Talos.walk": "Talos.default", "HumanoidTorque.run": "HumanoidTorque.default",
              "UnitreeH1.run": "UnitreeH1.default", "UnitreeG1.walk": "UnitreeG1.default", G.MESH: "mesh_feet", G.MUSCLE: "HumanoidMuscle.default",
              G.MUSCLE_NOPAIRS: "HumanoidMuscle.default.nopairs"}
FIELDS = ("family", "nv", "nu", "nobs", "max_links", "max_contacts", "npair", "na", "cm_used", "all_pyr3", "root_xyz")
# one blob per family: the derived facts, recorded from the parent's lm_model_create the same way (nobs: the neutral task's, 2 nv)
DERIVED = {
    "UnitreeA1.torque": (0, 18, 12, 36, 3, 3, 522, 0, 1664, 0, 1),
    "Atlas.default": (2, 16, 10, 32, 5, 8, 0, 0, 2368, 1, 1),
    "Talos.default": (4, 18, 12, 36, 5, 8, 0, 0, 2048, 1, 1),
    "HumanoidMuscle.default.nopairs": (5, 19, 92, 38, 5, 4, 0, 92, 2176, 1, 0),
    "UnitreeA1.torque.rk4": (6, 18, 12, 36, 3, 3, 522, 0, 1664, 0, 1),
    "UnitreeG1.default": (7, 29, 23, 58, 6, 8, 915, 0, 1920, 1, 1),
    "HumanoidTorque.default": (8, 19, 13, 38, 5, 8, 693, 0, 2240, 1, 0),
    "UnitreeH1.default": (9, 17, 11, 34, 5, 8, 135, 0, 2048, 1, 1),
    "HumanoidMuscle.default": (10, 19, 92, 38, 5, 8, 693, 92, 2240, 1, 0),
    "mesh_feet": (11, 23, 17, 46, 7, 8, 850, 0, 2176, 1, 0),
}
# optional tables of those blobs: the cuts are header, header + constant table and one per table
TABLES = {"UnitreeA1.torque": 2, "Atlas.default": 0, "Talos.default": 2, "HumanoidMuscle.default.nopairs": 3, "UnitreeA1.torque.rk4": 2, "UnitreeG1.default": 5,
          "HumanoidTorque.default": 5, "UnitreeH1.default": 5, "HumanoidMuscle.default": 6, "mesh_feet": 5}


def _neutral_task(m, **kw):
    """A task that needs nothing but the model: every dof observed, every actuator an action, no goal, no termination, no reward."""
    dofs, nu = list(range(int(m.nv))), int(m.nu)
    return dict(nobs=2 * len(dofs), qpos_obs_idx=dofs, qvel_obs_idx=dofs, n_goal=0, grf_groups=[], act_ctrl_idx=list(range(nu)), act_mean=np.zeros(nu),
                act_delta=np.ones(nu), term=[], reward_type=0, reward_params=[], n_substeps=10, **kw)


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    """The program, built once, and every blob as a raw float64 file: run(mode, names) -> its output lines."""
    tmp = tmp_path_factory.mktemp("model_parse")
    exe = str(tmp / "model_parse")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "model_parse_main.cpp")])
    paths = sorted(glob.glob(os.path.join(ASSETS, "*.model.npz")))
    assert sorted(os.path.basename(p)[:-len(".model.npz")] for p in paths) == sorted(FAMILIES)          # the 35 shipped models
    sources = [(os.path.basename(p)[:-len(".model.npz")], p, {}) for p in paths]
    sources += [("mesh_feet", MESH, {}), ("HumanoidMuscle.default.nopairs", os.path.join(ASSETS, "HumanoidMuscle.default.model.npz"), dict(self_collisions=False))]
    blobs = {}
    for name, path, kw in sources:
        m = mjcf.CompiledModel.load(path)
        blobs[name] = np.ascontiguousarray(lowering.lower(m, _neutral_task(m, **kw))[0], dtype=np.float64)
    for src in ("UnitreeA1.torque", "UnitreeG1.legs"):
        blobs[src + ".rk4"] = blobs[src].copy()
        blobs[src + ".rk4"][lowering.H_INTEGRATOR] = 1.0
    import generic_family_common as GF
    for name, (src, edit, _) in EDITED.items():
        m = mjcf.CompiledModel.load(os.path.join(ASSETS, src + ".model.npz"))
        getattr(GF, edit)(m)
        blobs[name] = np.ascontiguousarray(lowering.lower(m, _neutral_task(m))[0], dtype=np.float64)
    for name, blob in blobs.items():
        blob.tofile(str(tmp / (name + ".bin")))

    def run(mode, names=()):
        r = subprocess.run([exe, mode] + [str(tmp / (n + ".bin")) for n in names], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        lines = r.stdout.splitlines()
        assert lines[-1] == "model parse: ok"
        return lines[:-1]

    run.blobs = blobs
    return run


def _facts(line):
    w = line.split()
    return w[0], tuple(int(w[2 + 2 * i]) for i in range(len(FIELDS)))


def test_family_of_every_shipped_model(parse):
    want = dict(FAMILIES, **EXTRA)
    got = dict((name, facts[0]) for name, facts in map(_facts, parse("parse", sorted(want))))
    assert got == want
    assert len(FAMILIES) == 35 and sorted(set(want.values())) == [-1, 0, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    for task, fam in G.FAMILY.items():
        assert want[SAME_ROBOT[task]] == fam, task


def test_generic_family_serves_each_of_its_models_with_the_stated_instance(parse):
    """Every blob of family 6: links and contact slots per chain and the integrator of the instance that lm_family.hip launches
    (generic_instance), cone read at run time, no muscles, no pair pass. The models no kernel is compiled for are refused with a reason
    that names it — the muscle model because the generic kernels have no muscles."""
    want = dict(FAMILIES, **EXTRA)
    generic = sorted(k for k, v in want.items() if v == 6)
    assert generic == sorted(GENERIC_INSTANCE)
    for ln in parse("instances", generic):
        w = ln.split()
        assert tuple(int(w[i]) for i in (2, 4, 6, 8, 10, 12, 14, 16)) == (6, 1) + GENERIC_INSTANCE[w[0]][:2] + (GENERIC_INSTANCE[w[0]][2], -1, 0, 0), ln
    assert sorted(set(GENERIC_INSTANCE.values())) == [(3, 4, 0), (3, 4, 1), (5, 8, 0), (5, 8, 1)]          # every instance is reached
    refused = dict((ln.split()[0], ln.split("refused: ", 1)[1]) for ln in parse("instances", sorted(k for k, v in want.items() if v == -1)))
    assert sorted(refused) == ["HumanoidMuscle.default.elliptic", "UnitreeG1.default.elliptic", "UnitreeG1.legs.rk4"]
    assert "have no muscles" in refused["HumanoidMuscle.default.elliptic"] and "muscle models need" in refused["HumanoidMuscle.default.elliptic"]
    assert all("chains of six links" in refused[k] for k in ("UnitreeG1.default.elliptic", "UnitreeG1.legs.rk4"))


def test_emulator_picks_the_librarys_instance_for_every_blob(parse):
    """tests/emu/emu.cpp chooses through pick_family and family() of lm_families.h, like lm_model_create and the launch code: for every
    blob here the emulator's regular instantiation is the library's — family, links, slots, integrator, muscles, pair pass, and the
    compiled-in cone — and a model without a family has none."""
    from emu import pyemu
    lib = C.CDLL(pyemu.build())
    want = dict(FAMILIES, **EXTRA)
    n = 0
    for ln in parse("instances", sorted(want)):
        w = ln.split()
        out = (C.c_int * 8)()
        blob = parse.blobs[w[0]]
        lib.emu_instance(blob.ctypes.data_as(C.c_void_p), 0, out)
        if want[w[0]] < 0:
            assert w[2] == "-1" and (out[0], out[1]) == (-1, 0), ln
        else:
            assert list(out) == [int(w[i]) for i in (2, 4, 6, 8, 10, 12, 14, 16)], (ln, list(out))
            n += 1
    assert n == len(want) - 3


def test_derived_task_facts_of_one_model_per_family(parse):
    got = dict(map(_facts, parse("parse", sorted(DERIVED))))
    assert got == DERIVED
    assert sorted(v[0] for v in DERIVED.values()) == [0, 2, 4, 5, 6, 7, 8, 9, 10, 11]


def test_truncated_blobs_are_refused_with_a_message(parse):
    """One blob per family cut to the header, to header + constant table and one double short of the end of each optional table it has:
    every cut is refused with a message (the program checks each; a read past the end of a cut would be a sanitizer report)."""
    lines = parse("cuts", sorted(TABLES))
    for name, tables in TABLES.items():
        assert "%s: %d cuts refused" % (name, 2 + tables) in lines, name
        mine = [ln for ln in lines if ln.startswith(name + " cut at ")]
        assert len(mine) == 2 + tables and all(ln.split("): ", 1)[1].startswith("chain model ") for ln in mine), mine


def test_family_table_agrees_with_the_library_on_every_family_and_kind(parse):
    """has_kind(family, kind) of lm_families.h — what the launches and lm_batch_set_layout go by — against lm_lds_bytes of the built
    library, which asks the launch code of the family's objects: the same answer for every pair, the absent families included."""
    from loco_mujoco_amd.backend import load_library
    lib = load_library()
    rows = dict((int(ln.split()[1]), [int(x) for x in ln.split()[3:]]) for ln in parse("kinds"))
    assert sorted(rows) == list(range(-1, 13)) and all(len(r) == 13 for r in rows.values())
    for fam, row in rows.items():
        for kind, present in enumerate(row):
            s, d = C.c_int(0), C.c_int(0)
            ok = lib.lm_lds_bytes(fam, kind, 4, 2048, C.byref(s), C.byref(d)) == 0
            assert ok == bool(present), (fam, kind)
            assert not ok or (s.value > 0 and d.value > 4 * 2048)


def test_counts_that_would_read_outside_the_buffer_are_refused(parse):
    """The three refusals the parser adds, at their boundaries (the program checks each answer; every blob sits in a buffer of exactly
    its size): a chain's geom count and link count are accepted up to the largest value whose reads stay inside the blob / the constant
    table and refused from the next on; a geom-pair count or offset that is negative, not a number, huge or beyond the blob is refused."""
    lines = parse("pokes", ["Atlas.default", "UnitreeA1.torque", "HumanoidTorque.default"])
    assert sum("(inside): parsed" in ln for ln in lines) == 10          # geoms: the two pyramidal blobs x 2 chains; links: 3 x 2
    assert sum("geom count runs past" in ln for ln in lines) == 8 and sum("link count runs past" in ln for ln in lines) == 12
    assert sum("(count): chain model lacks" in ln for ln in lines) == 8 and sum("(offset): chain model lacks" in ln for ln in lines) == 10
