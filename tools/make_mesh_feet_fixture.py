"""
Writes the mesh-foot HumanoidTorque model the tests use (``tests/golden/humanoid_torque_mesh_feet.model.npz``): the reference's
``humanoid_torque.xml`` after the environment's XML surgery for ``use_box_feet=False, disable_arms=True`` (arm joints, motors and
wrist constraints removed, arms re-oriented; the subtalar / mtp joints, their motors and their four joint equality constraints kept),
compiled with the feet colliding as the bone meshes' convex hulls. Run in the build container only; no test reads the checkout.

  python tools/make_mesh_feet_fixture.py --ref /path/to/loco-mujoco
"""

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from loco_mujoco_amd import lowering                                  # noqa: E402
from loco_mujoco_amd.environments.humanoids import HumanoidTorque     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a loco-mujoco checkout")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "humanoid_torque_mesh_feet.model.npz"))
    args = ap.parse_args()
    xml = Path(args.ref) / "loco_mujoco" / "environments" / "data" / "humanoid" / "humanoid_torque.xml"
    env = HumanoidTorque(use_box_feet=False, xml_path=xml)
    m = env._model
    m.save(args.out)
    cmod, info = lowering.lower(m, env._device_task())
    print("mesh-foot HumanoidTorque: nv %d nu %d, %d chains of up to %d links, %d equality rows (%s), %s, %d hull vertices -> %s"
          % (m.nv, m.nu, info["n_chains"], info["max_links"], info.get("equality_rows", 0), ", ".join(m.eq_names),
             info.get("self_collision_tables"), info["mesh_vertices"], args.out))


if __name__ == "__main__":
    main()
