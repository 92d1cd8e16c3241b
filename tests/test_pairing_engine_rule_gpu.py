"""The launcher's own choice of pairing engine on the device against the host-only rule (csrc/h2v_pairing_engine.hpp): for
(in-flight hint, batch size) on both sides of the rule's borders that a small batch can reach, an ordinary workspace reports the
engine that the model program (tests/cpp/h2v_pairing_engine.cpp) names for this device's SIMD count, and the verdicts are the
construction's.  On 1024 SIMDs the six cases are wide, wide, coop 32, twelve, wide and coop 32.  The six-lane engine's border at
3 x #SIMDs proofs is left to the table (tests/test_pairing_engine_model.py) and to the tests that force that engine."""
import subprocess

import pytest

from tests.test_gpu_parity import _permute, be  # noqa: F401  (be: the module's backend fixture)
from tests.test_pairing_engine_model import build_model_program

pytestmark = pytest.mark.gpu


def test_the_launchers_choice_is_the_models(be, tmp_path):
    import torch
    from plutus_halo2_verifier_gen_amd import plan as PL, synth, vk as V
    S = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    program = build_model_program(tmp_path, sanitizers=False)
    vk, td = V.simple_mul_vk()
    pl = PL.compile_plan(vk)
    dp = be.DevicePlan(pl.to_bytes(), 0)
    n_max, n_pi = S // 2 + 1, vk.n_public_inputs
    batch = synth.forge_batch(vk, td, n_max, seed=91, plan=pl, workers=16)
    batch = synth.with_rejects(pl, batch, n_pi, fraction=0.03, seed=92, kinds=list(synth.CORRUPTIONS))
    assert 0 < sum(batch.expected) < n_max
    seen = set()
    for hint, n in ((1, 1), (8, S // 16), (8, S // 16 + 1), (8, 3 * S // 8), (4, S // 2), (4, S // 2 + 1)):
        # (no option; the six-lane table's presence plays no part below 3 x #SIMDs proofs)
        r = subprocess.run([program, "--simds", str(S), "--case", str(n), str(hint), "0", "1"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        case, answer = r.stdout.strip().split(" : ")
        assert case == "pipe %d %d 1 0" % (n, hint)
        engine, grid, lanes = answer.split()
        ws = be.Workspace(dp, n_max)
        if hint != 1:
            ws.hint_in_flight(hint)
        pre = batch if n == n_max else _permute(batch, list(range(n)), n_pi)
        got = dp.verify_batch(pre.proofs, pre.proof_off, pre.instances, pre.committed, ws=ws)
        print("hint %d, n %d: the model says %s (%s lanes), the workspace reports %d" % (hint, n, engine, lanes, ws.timings().pairing_lanes_per_proof))
        assert ws.timings().pairing_lanes_per_proof == int(lanes), (hint, n, engine)
        assert list(got) == batch.expected[:n], (hint, n, engine)
        ws.close()
        seen.add(engine)
    assert len(seen) >= 3      # (wide, coop 32 and twelve on an MI355X: the cases do cross borders)
