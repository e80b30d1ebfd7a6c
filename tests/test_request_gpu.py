"""GD4D_REQUEST=1: an eager decoder request issued by ONE host call (fused_decoder.RequestProgram over gd4d_decoder_request_run)
against the same call with the switch off.  The program enqueues the kernels of the Python loop with the same grids and
arguments in the same order on the same two streams, so every comparison is torch.equal - bit for bit.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CAMS, LAYERS = 24, 6
HOST_ONLY = ('_bytes', 'gd4d_error_string', 'gd4d_last_hip_error', 'gd4d_abi_version', 'gd4d_decoder_request_describe',
             'gd4d_decoder_request_create', 'gd4d_decoder_request_destroy')


def _pyramid(seed):
    from graph_detr4d_amd import synthetic
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [torch.randn(1, CAMS, 256, h, w, device='cuda', generator=g) for h, w in synthetic.R50_LEVELS]


def _metas(frame_shift=0.5):
    from graph_detr4d_amd import synthetic
    return synthetic.make_img_metas(synthetic.camera_rig(CAMS // 6, frame_shift=frame_shift), batch=1)


@pytest.fixture(scope='module')
def scene():
    """Six layers, 24 cameras, the R50 pyramid, 900 queries - bench.py's model; made once, never modified by a test that does not
    restore it."""
    import bench
    import graph_detr4d_amd as G
    tr, regs = bench.build_decoder(G, CAMS, LAYERS, 'fp32', 1002)
    tr, regs = tr.cuda(), regs.cuda()
    qe = torch.randn(900, 512, generator=torch.Generator().manual_seed(5)).cuda()
    return dict(tr=tr, regs=regs, feats=_pyramid(77), qe=qe, metas=_metas())


def _call(monkeypatch, request, tr, feats, qe, regs, metas, **kw):
    monkeypatch.setenv('GD4D_REQUEST', '1' if request else '0')
    with torch.no_grad():
        states, init_ref, refs = tr(feats, qe, reg_branches=regs, img_metas=metas, **kw)
    torch.cuda.synchronize()
    return states, refs


def _same(monkeypatch, tr, feats, qe, regs, metas, **kw):
    from graph_detr4d_amd import fused_decoder
    want = _call(monkeypatch, False, tr, feats, qe, regs, metas, **kw)
    entered = []
    orig = fused_decoder.RequestProgram.run
    monkeypatch.setattr(fused_decoder.RequestProgram, 'run', lambda self, *a: (entered.append(1), orig(self, *a))[1])
    got = _call(monkeypatch, True, tr, feats, qe, regs, metas, **kw)
    again = _call(monkeypatch, True, tr, feats, qe, regs, metas, **kw)                   # the program serves a second request
    monkeypatch.setattr(fused_decoder.RequestProgram, 'run', orig)
    assert entered == [1, 1], 'the call did not take the request program'
    for w, g, a in zip(want, got, again):
        assert w.shape == g.shape and torch.isfinite(w).all()
        assert torch.equal(w, g) and torch.equal(w, a)
    return want


def test_request_equals_eager_nchw(scene, monkeypatch):
    states, refs = _same(monkeypatch, scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])
    assert states.shape == (LAYERS, 900, 1, 256) and refs.shape == (LAYERS, 1, 900, 3)


def test_request_equals_eager_channels_last(scene, monkeypatch):
    feats = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in scene['feats']]
    _same(monkeypatch, scene['tr'], feats, scene['qe'], scene['regs'], scene['metas'])


def test_request_equals_eager_last_layer_only(scene, monkeypatch):
    dec = scene['tr'].decoder
    monkeypatch.setattr(dec, 'return_intermediate', False)
    states, refs = _same(monkeypatch, scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])
    assert states.shape == (900, 1, 256) and refs.shape == (1, 900, 3)


def test_request_equals_eager_without_reg_branches(scene, monkeypatch):
    _same(monkeypatch, scene['tr'], scene['feats'], scene['qe'], None, scene['metas'])


def test_request_equals_eager_hdetr_block_mask(scene, monkeypatch):
    """H-DETR: 900 one-to-one + 1800 one-to-many queries, each group attending to itself only."""
    qe = torch.randn(2700, 512, generator=torch.Generator().manual_seed(6)).cuda()
    mask = torch.zeros(2700, 2700, dtype=torch.bool, device='cuda')
    mask[:900, 900:] = True
    mask[900:, :900] = True
    states, _ = _same(monkeypatch, scene['tr'], scene['feats'], qe, scene['regs'], scene['metas'], attn_masks=[mask, None])
    assert states.shape == (LAYERS, 2700, 1, 256)


@pytest.mark.parametrize('switch,value', [('GD4D_POS_ENCODER', 'dual'), ('GD4D_COARSE', '0'), ('GD4D_FIRST_PROJ', 'side'),
                                          ('GD4D_MHA_FP32', '1')])
def test_request_equals_eager_under_route_switch(scene, monkeypatch, switch, value):
    monkeypatch.setenv(switch, value)
    _same(monkeypatch, scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])


def test_a_recording_reads_schedule_switches_only(scene, monkeypatch):
    """The program's key holds the raw values of switches.SCHEDULE; the read log of a recording (RequestProgram.switches_read: every
    switch the recorded code asked the environment) must lie inside that set - a switch read there and missing from the key would
    let a recorded launch sequence be replayed after the switch changed."""
    from graph_detr4d_amd import fused_decoder, switches
    programs = []
    orig = fused_decoder.RequestProgram.__init__
    monkeypatch.setattr(fused_decoder.RequestProgram, '__init__', lambda self, *a: (orig(self, *a), programs.append(self))[0])
    monkeypatch.setenv('GD4D_COPY_CUS', '200')             # (a key no other test of this file uses: this call records)
    _call(monkeypatch, True, scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])
    assert len(programs) == 1
    read = programs[0].switches_read
    print('switches read while recording:', sorted(read))
    assert read and read <= set(switches.SCHEDULE), sorted(read - set(switches.SCHEDULE))
    assert {'GD4D_AGG', 'GD4D_COPY_CUS', 'GD4D_POS_ENCODER', 'GD4D_MHA_FP32'} <= read      # (LateValues and run_single were recorded)


def test_all_exact_is_part_of_the_program_key(scene, monkeypatch):
    """`with ops.all_exact():` selects other chain descriptors without touching the environment: a request inside it must not be
    served by the program recorded outside it."""
    from graph_detr4d_amd import ops
    args = (scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])
    x3 = _same(monkeypatch, *args)
    with ops.all_exact():
        exact = _same(monkeypatch, *args)
    assert not torch.equal(x3[0], exact[0])
    assert torch.equal(_same(monkeypatch, *args)[0], x3[0])


def test_mixed_level_layouts_take_the_eager_path(scene, monkeypatch):
    """Two dense and two channels-last levels: LateValues copies such a list with torch ops, which are no steps of a program -
    the call is declined (and, repeated on other data, does not read the first call's copy)."""
    from graph_detr4d_amd import fused_decoder
    monkeypatch.setattr(fused_decoder.RequestProgram, '__init__', lambda self, *a: pytest.fail('a program was recorded'))
    for seed in (77, 78):
        feats = _pyramid(seed)
        feats[2:] = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in feats[2:]]
        want = _call(monkeypatch, False, scene['tr'], feats, scene['qe'], scene['regs'], scene['metas'])
        got = _call(monkeypatch, True, scene['tr'], feats, scene['qe'], scene['regs'], scene['metas'])
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


def test_handoffs_turned_off_rerecord_the_program(scene, monkeypatch):
    """ops.check_handoff turns the device's hand-offs off after a time-out; the eager loop then builds its steps without them, and so
    must the next request (a program recorded before would wait on the same hand-off again)."""
    from graph_detr4d_amd import fused_decoder, ops
    args = (scene['tr'], scene['feats'], scene['qe'], scene['regs'], scene['metas'])
    want = _same(monkeypatch, *args)
    state = ops._handoff_state(scene['qe'].device)
    if not state['placement']:
        pytest.fail('the hand-off schedule is expected to be the default on this device')
    used = []
    run = fused_decoder.RequestProgram.run
    try:
        state['placement'] = False
        monkeypatch.setattr(fused_decoder.RequestProgram, 'run', lambda self, *a: (used.append(self), run(self, *a))[1])
        got = _call(monkeypatch, True, *args)
        monkeypatch.setattr(fused_decoder.RequestProgram, 'run', run)
        dual = _call(monkeypatch, False, *args)
    finally:
        state['placement'] = True
    assert torch.equal(got[0], dual[0]) and torch.equal(got[0], want[0])
    # [chain A | reg, refine, position_encoder] and chain B' alone: no two-program launch carries the guest any more
    assert len(used) == 1 and not used[0].polls


def test_other_reg_branches_are_not_served_the_recorded_ones(scene, monkeypatch):
    import copy
    args = (scene['tr'], scene['feats'], scene['qe'])
    first = _same(monkeypatch, *args, scene['regs'], scene['metas'])
    regs = copy.deepcopy(scene['regs'])
    with torch.no_grad():
        for r in regs:
            r[-1].weight.mul_(3.0)
    second = _same(monkeypatch, *args, regs, scene['metas'])
    assert not torch.equal(first[1], second[1])
    assert torch.equal(_same(monkeypatch, *args, scene['regs'], scene['metas'])[1], first[1])


def test_one_program_serves_requests_at_other_addresses(scene, monkeypatch):
    """The binding test: three consecutive requests on fresh tensors at other addresses with other lidar2img matrices go through
    ONE program, and each equals its eager result."""
    from graph_detr4d_amd import fused_decoder
    tr, regs = scene['tr'], scene['regs']
    _call(monkeypatch, True, tr, scene['feats'], scene['qe'], regs, scene['metas'])
    programs = dict(fused_decoder._PROGRAMS[tr.decoder])
    held, addresses = [], set()
    for k in range(3):
        feats = _pyramid(100 + k)
        qe = torch.randn(900, 512, generator=torch.Generator().manual_seed(50 + k)).cuda()
        metas = _metas(frame_shift=0.3 + 0.2 * k)
        held.append((feats, qe))                                         # (kept: the next request cannot land on these addresses)
        addresses.add((feats[0].data_ptr(), qe.data_ptr()))
        got = _call(monkeypatch, True, tr, feats, qe, regs, metas)
        want = _call(monkeypatch, False, tr, feats, qe, regs, metas)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(got[0], _call(monkeypatch, False, tr, scene['feats'], scene['qe'], regs, scene['metas'])[0])
    assert len(addresses) == 3
    after = fused_decoder._PROGRAMS[tr.decoder]
    assert set(after) == set(programs) and all(after[k] is programs[k] for k in programs), 'a request rebuilt the program'


def test_a_changed_parameter_rebuilds_the_program(scene, monkeypatch):
    from graph_detr4d_amd import fused_decoder, ops
    tr, regs, feats, qe, metas = (scene[k] for k in ('tr', 'regs', 'feats', 'qe', 'metas'))
    before = _call(monkeypatch, True, tr, feats, qe, regs, metas)
    builds = []
    orig = fused_decoder.RequestProgram.__init__
    monkeypatch.setattr(fused_decoder.RequestProgram, '__init__', lambda self, *a: (builds.append(1), orig(self, *a))[1])
    weight = tr.decoder.layers[2].attentions[1].value_proj.weight
    saved = weight.detach().clone()
    try:
        with torch.no_grad():
            weight.mul_(1.25)
        ops.invalidate_chain_images()
        got = _call(monkeypatch, True, tr, feats, qe, regs, metas)
        assert builds == [1]
        want = _call(monkeypatch, False, tr, feats, qe, regs, metas)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(got[0], before[0])
    finally:
        with torch.no_grad():
            weight.copy_(saved)
        ops.invalidate_chain_images()
    assert torch.equal(_call(monkeypatch, True, tr, feats, qe, regs, metas)[0], before[0])


def test_a_captured_forward_does_not_enter_the_program(scene, monkeypatch):
    from graph_detr4d_amd import fused_decoder
    tr, regs, feats, qe, metas = (scene[k] for k in ('tr', 'regs', 'feats', 'qe', 'metas'))
    stream = torch.cuda.Stream()

    def captured(request):
        monkeypatch.setenv('GD4D_REQUEST', '1' if request else '0')
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
            out = tr(feats, qe, reg_branches=regs, img_metas=metas)
        graph.replay()
        torch.cuda.synchronize()
        return out[0].clone(), out[2].clone()

    monkeypatch.setenv('GD4D_REQUEST', '0')
    with torch.no_grad(), torch.cuda.stream(stream):
        tr(feats, qe, reg_branches=regs, img_metas=metas)                    # (uploads the matrices; a capture cannot)
    torch.cuda.synchronize()
    want = captured(False)

    def refuse(*a, **k):
        raise AssertionError('RequestProgram entered while the stream is capturing')
    monkeypatch.setattr(fused_decoder, 'request_forward', refuse)
    got = captured(True)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


class Counting:
    """The library with every launching entry point counted."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if any(name.endswith(h) for h in HOST_ONLY):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def _decoder_call(scene, monkeypatch, request):
    from graph_detr4d_amd import fused_decoder
    tr = scene['tr']
    monkeypatch.setenv('GD4D_REQUEST', '1' if request else '0')
    query_pos, query = torch.split(scene['qe'], 256, dim=1)
    with torch.no_grad():
        ref = fused_decoder.initial_reference(tr.reference_points, query_pos)
        torch.cuda.synchronize()
        return lambda: tr.decoder(query=query.unsqueeze(1), key=None, value=scene['feats'], query_pos=query_pos.unsqueeze(1),
                                  reference_points=ref, reg_branches=scene['regs'], img_metas=scene['metas'])


def test_describe_lists_what_the_eager_loop_launches_and_a_request_is_one_call(scene, monkeypatch):
    from graph_detr4d_amd import _lib, fused_decoder
    real = _lib.load()
    with torch.no_grad():
        eager, request = _decoder_call(scene, monkeypatch, False), _decoder_call(scene, monkeypatch, True)
        monkeypatch.setenv('GD4D_REQUEST', '0')
        want = eager()                                                         # (weight images, probes: made before anything is counted)
        monkeypatch.setenv('GD4D_REQUEST', '1')
        got = request()
        torch.cuda.synchronize()
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
        counting = Counting(real)
        monkeypatch.setattr(_lib, '_lib', counting)
        monkeypatch.setenv('GD4D_REQUEST', '0')
        ran = []
        orig = fused_decoder.run_single
        monkeypatch.setattr(fused_decoder, 'run_single', lambda *a, **k: (ran.append(1), orig(*a, **k))[1])
        eager()
        launched, counting.calls = counting.calls, []
        assert ran == [1] and len(launched) >= 4 * LAYERS
        monkeypatch.setenv('GD4D_REQUEST', '1')
        used = []
        run = fused_decoder.RequestProgram.run
        monkeypatch.setattr(fused_decoder.RequestProgram, 'run', lambda self, *a: (used.append(self), run(self, *a))[1])
        request()
        assert counting.calls == ['gd4d_decoder_request_run'] and ran == [1] and len(used) == 1
        torch.cuda.synchronize()
    described = used[0].describe()
    assert [n for n in described if n.startswith('gd4d_')] == launched
    assert {n for n in described if not n.startswith('gd4d_')} == {'hipEventRecord', 'hipStreamWaitEvent'}
