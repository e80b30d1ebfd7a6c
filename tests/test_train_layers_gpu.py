"""Every layer of ONE decoder training call's BACKWARD against the fp64 oracle, stepped (GPU only).

The training step bench.py --mode train times - fused_train.DecoderTrainFunction: 6 layers, 900 queries (56 full row blocks + a
4-row partial block), 24 cameras, the R50 pyramid, reg-branch refinement, queued weight gradients, record fills riding as guest
workgroups, the pyramid gradient of all layers reduced in one pass - runs once; its decisions are recorded
(tests/train_step.DecisionSpy: visibility mask, bilinear corners - read back from the plan's pairs form and required equal to the
ones recomputed from uv -, post-ReLU buffers, dropout keep masks) and the oracle is stepped backward layer by layer on the call's
own states / refs with those decisions, in fp64 (tests/train_step.py).  With every discontinuity forced what is left is
rounding, so every parameter tensor of every layer, reference_points, query_embed and the pyramid gradient are held to
relative Frobenius error <= 1e-3 and every output row / query row / (level, camera) block to <= 1e-2 (an entry of a bias or
LayerNorm gradient against the tensor's RMS entry: train_step.errors); the decision-mismatch
report bounds how often the fp64 oracle's own choice disagrees with a forced one.  The table (A: implementation vs fp64 oracle,
C: the fp32 oracle with the same decisions vs fp64 - the yardstick) is tools/stepped_backward_parity.py's
(docs/measurements_r10.md)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('stepped_backward_parity', os.path.join(ROOT, 'tools', 'stepped_backward_parity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('case', ['refine', 'no-refine', 'dropout'])
def test_training_backward_900q_24cams_six_layers_steps_the_fp64_oracle(case):
    """refine: eval mode with reg branches (the bench's default); no-refine: no reg branches, so the reference points' gradient
    flows through every layer's plan backward and the loss also probes inter_refs; dropout: train mode (p = 0.1 at the five
    sites), seeds fixed through fused_train.draw_seeds."""
    from train_step import mismatch_failures
    tool = _tool()
    res = tool.run_case(case)
    print()
    print(tool.table(res))
    assert res['calls'] == 1, 'the call must take the row-chain training path'
    assert res['kinds'] == ['cross_attn_plan_fwd'] * 6, res['kinds']
    # the corners the oracle is forced onto are the ones the gather used: the plan's pairs, every visible sample and level
    assert all(m == 0 and bad == 0 and tot > 0 for m, bad, tot in res['plan_checks']), res['plan_checks']
    assert res['init_ref_err'] < 1e-6, res['init_ref_err']
    assert not mismatch_failures(res['mismatch']), res['mismatch']
    assert not res['fails_A'], res['fails_A']
    # the yardstick: fp32 arithmetic itself fits the same bounds
    assert not res['fails_C'], res['fails_C']
