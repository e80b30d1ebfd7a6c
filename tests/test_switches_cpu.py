"""The GD4D_* environment switches (graph_detr4d_amd/switches.py): what every accepted value means, what is refused, that reads are per
call, that the package reads the environment nowhere else, and that README.md's table and the request program's key follow the
registry.  The truth table below is written from the switches' documented meaning, not from the registry."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'graph-detr4d_amd')

ON, OFF = {None: True, '': True, '0': False, '1': True}, {None: False, '': False, '0': False, '1': True}
TRUTH = {                               # switch -> {raw value (None: unset): what the reader answers}
    **{'GD4D_' + n: ON for n in ('FUSED_DECODER', 'TRAIN_CHAINS', 'QUERY_ORDER', 'AUX_STREAM', 'COARSE', 'HEAD_CHAINS', 'PE_FRUSTUM',
                                 'PE_FUSED', 'TRAIN_REG_BESIDE')},
    'GD4D_POS_ENCODER': dict(ON, dual=False, chainb=True),
    **{'GD4D_' + n: OFF for n in ('REQUEST', 'TORCH_OPS', 'MHA_FP32', 'CHAIN_ALL_EXACT')},
    'GD4D_PROJECT': {None: 'late', '': 'late', 'late': 'late', 'early': 'early'},
    'GD4D_TRAIN_VALUES': {None: 'raw', '': 'raw', 'raw': 'raw', 'projected': 'projected'},
    'GD4D_AGG': {None: 'sliced', '': 'sliced', 'sliced': 'sliced', 'rows': 'rows'},
    'GD4D_PLAN': {None: 'items', '': 'items', 'items': 'items', 'pairs': 'pairs'},
    'GD4D_FIRST_PROJ': {None: 'main', '': 'main', 'main': 'main', 'side': 'side'},
    'GD4D_FILLS_RIDE': {None: 'chain', '': 'chain', 'chain': 'chain', 'mha': 'mha'},
    'GD4D_VALUE_LAYOUT': {None: None, '': None, 'pixel': 'pixel', 'head': 'head'},
    'GD4D_COPY_CUS': {None: None, '': None, '0': 0, '192': 192},
    'GD4D_PIPELINE_CUS': {None: None, '': None, '0': 0, '64': 64},
    'GD4D_COARSE_MAX_ROWS': {None: 65536, '': 65536, '0': 0, '200000': 200000},
    'GD4D_PREPROJECT': {None: 'auto', '': 'auto', 'auto': 'auto', '0': '0', '1': '1', 'stream': 'stream', 'g2': 'g2', 'g2,2,2': 'g2,2,2',
                        'whatever': 'whatever'},
    'GD4D_LIB_PATH': {None: None, '': None, '/somewhere/libgd4d.so': '/somewhere/libgd4d.so'},
    'GD4D_DIST_BACKEND': {None: 'nccl', '': 'nccl', 'nccl': 'nccl', 'gloo': 'gloo'},
    'GD4D_PREFLIGHT_MB': {None: '22,140,330', '': '22,140,330', '2,8': '2,8'},
}
# the ten names the request program's key held before the registry existed: the schedule set may grow, never lose one of these
SCHEDULE_FLOOR = {'GD4D_POS_ENCODER', 'GD4D_COARSE', 'GD4D_FIRST_PROJ', 'GD4D_MHA_FP32', 'GD4D_AGG', 'GD4D_PLAN', 'GD4D_PROJECT',
                  'GD4D_COPY_CUS', 'GD4D_COARSE_MAX_ROWS', 'GD4D_QUERY_ORDER'}
READER = {'flag': 'flag', 'choice': 'choice', 'int': 'integer', 'path': 'path', 'spec': 'spec'}


def _reader(sw):
    from graph_detr4d_amd import switches
    return getattr(switches, READER[sw.kind])


def _set(monkeypatch, name, raw):
    if raw is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, raw)


def test_every_accepted_value_means_what_the_table_says(monkeypatch):
    from graph_detr4d_amd import switches
    assert set(TRUTH) == set(switches.REGISTRY)
    for name, sw in switches.REGISTRY.items():
        accepted = {'flag': ['0', '1'] + list(sw.values or ()), 'choice': list(sw.values or ())}.get(sw.kind, [])
        assert {None, ''} | set(accepted) <= set(TRUTH[name]), f'{name}: an accepted value is missing from the truth table'
        for raw, want in TRUTH[name].items():
            _set(monkeypatch, name, raw)
            got = _reader(sw)(name)
            assert got == want and type(got) is type(want), f'{name}={raw!r}: {got!r}, expected {want!r}'


@pytest.mark.parametrize('name,raw,accepted', [('GD4D_TORCH_OPS', 'true', '0, 1'), ('GD4D_TRAIN_REG_BESIDE', 'dual', '0, 1'),
                                               ('GD4D_POS_ENCODER', 'duall', 'chainb'), ('GD4D_PROJECT', 'lat', 'late, early'),
                                               ('GD4D_AGG', 'slice', 'sliced, rows'), ('GD4D_COPY_CUS', '19x', 'integers'),
                                               ('GD4D_COARSE_MAX_ROWS', '64k', 'integers')])
def test_a_misspelt_value_is_refused_by_name(monkeypatch, name, raw, accepted):
    from graph_detr4d_amd import switches
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.setenv(name, raw)
    with pytest.raises(Gd4dError) as e:
        _reader(switches.REGISTRY[name])(name)
    assert name in str(e.value) and repr(raw) in str(e.value) and accepted in str(e.value)


def test_preproject_stays_free_form(monkeypatch):
    from graph_detr4d_amd import functional as Fn, switches
    monkeypatch.setenv('GD4D_PREPROJECT', 'g2')
    assert switches.spec('GD4D_PREPROJECT') == 'g2'
    assert Fn.pipeline_groups('g2', 6) is None            # (does not add up to six layers: means `1`, one launch for all layers)


def test_reads_are_per_call_except_the_two_import_time_ones(monkeypatch):
    from graph_detr4d_amd import ops, switches
    monkeypatch.setenv('GD4D_AGG', 'rows')
    first = switches.choice('GD4D_AGG')
    monkeypatch.setenv('GD4D_AGG', 'sliced')
    assert (first, switches.choice('GD4D_AGG')) == ('rows', 'sliced')
    monkeypatch.setenv('GD4D_COARSE', '0')
    first = switches.flag('GD4D_COARSE')
    monkeypatch.delenv('GD4D_COARSE')
    assert (first, switches.flag('GD4D_COARSE')) == (False, True)
    assert {n for n, sw in switches.REGISTRY.items() if sw.read == 'import'} == {'GD4D_CHAIN_ALL_EXACT', 'GD4D_LIB_PATH'}
    seeded = ops.ALL_EXACT[0]
    monkeypatch.setenv('GD4D_CHAIN_ALL_EXACT', '0' if seeded else '1')
    assert ops.ALL_EXACT[0] is seeded                     # the seed was read when ops was imported; `with ops.all_exact():` changes it


def test_the_read_log_collects_what_a_recording_thread_reads(monkeypatch):
    from graph_detr4d_amd import _lib, switches
    assert switches._log.names is None          # off by default
    with switches.read_log() as names:
        switches.flag('GD4D_COARSE')                              # not recording: not collected
        with _lib.recording(object()):
            switches.choice('GD4D_AGG')
            switches.integer('GD4D_COPY_CUS')
        switches.flag('GD4D_REQUEST')
    assert names == {'GD4D_AGG', 'GD4D_COPY_CUS'} and switches._log.names is None
    with _lib.recording(object()):
        switches.flag('GD4D_COARSE')                              # recording with the log off: nothing kept anywhere
    assert names == {'GD4D_AGG', 'GD4D_COPY_CUS'}


def test_the_package_reads_the_environment_through_the_registry_only():
    from graph_detr4d_amd import switches
    read = {}
    for fn in sorted(os.listdir(PKG)):
        if not fn.endswith('.py') or fn == 'switches.py':
            continue
        src = open(os.path.join(PKG, fn)).read()
        if fn == 'dist.py':                               # the torch.distributed.run variables: not switches of the package
            assert set(re.findall(r"environ\.\w+\('(\w+)'", src)) == {'RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'}
            assert len(re.findall(r'\benviron\b|getenv', src)) == 5
        else:
            assert not re.search(r'\benviron\b|getenv', src), f'{fn} reads the environment itself'
        for reader, name in re.findall(r"switches\.(flag|choice|integer|path|spec)\('(GD4D_\w+)'\)", src):
            assert READER[switches.REGISTRY[name].kind] == reader, f'{fn}: {name} read as {reader}'
            read[name] = fn
        for name in re.findall(r"handoff_enabled\(\w+, '(GD4D_\w+)'\)", src):          # (a flag, handed to ops.handoff_enabled by name)
            assert switches.REGISTRY[name].kind == 'flag'
            read[name] = fn
    benchs = {n for n, sw in switches.REGISTRY.items() if sw.read == 'bench.py'}
    assert benchs == {'GD4D_DIST_BACKEND', 'GD4D_PREFLIGHT_MB'}
    assert set(read) == set(switches.REGISTRY) - benchs
    bench = open(os.path.join(ROOT, 'bench.py')).read()
    for name, default in re.findall(r"environ\.get\('(GD4D_\w+)', '([^']*)'", bench):   # the defaults bench.py spells out
        assert switches.default_text(switches.REGISTRY[name]) == default, name
    assert all(n in bench for n in benchs)


def test_readme_table_follows_the_registry():
    from graph_detr4d_amd import switches
    readme = open(os.path.join(ROOT, 'README.md')).read()
    rows = re.findall(r'^\| `(GD4D_\w+)` \| ([^|]*) \|', readme, flags=re.M)
    assert len(rows) == len(dict(rows))
    assert {n: d.strip().strip('`') for n, d in rows} == {n: switches.default_text(sw) for n, sw in switches.REGISTRY.items()}
    assert f'the complete list: {len(switches.REGISTRY)}\n' in readme


def test_the_schedule_set_keeps_the_ten_and_keys_their_raw_values(monkeypatch):
    from graph_detr4d_amd import switches
    assert SCHEDULE_FLOOR <= set(switches.SCHEDULE)
    assert all(switches.REGISTRY[n].schedule for n in switches.SCHEDULE)
    for name in switches.SCHEDULE:
        monkeypatch.delenv(name, raising=False)
    unset = switches.schedule_key()
    assert unset == (None,) * len(switches.SCHEDULE)
    monkeypatch.setenv('GD4D_FIRST_PROJ', 'side')
    assert switches.schedule_key() != unset and switches.schedule_key()[switches.SCHEDULE.index('GD4D_FIRST_PROJ')] == 'side'
