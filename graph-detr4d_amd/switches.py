"""The GD4D_* environment switches: the one place that names them.

The rule.  A switch is declared once, in the table below: name, kind, default, accepted values, one line of meaning, and whether
it selects the schedule a request program records.  The package reads a switch through this module's readers and nowhere else
(`flag`, `choice`, `integer`, `path`, `spec` - one per kind); README.md's table restates names and defaults, and
tests/test_switches_cpu.py holds both to this table.

  * Per-call reads.  A reader asks the environment at EVERY call and keeps nothing: tests, bench.py and the tools change switches
    while the process runs.
  * Two import-time reads.  GD4D_LIB_PATH (_lib.LIB_PATH) and GD4D_CHAIN_ALL_EXACT (the seed of ops.ALL_EXACT, which
    `with ops.all_exact():` changes afterwards) are read once, when their module is imported: `read='import'`.
  * One C-side read.  GD4D_MHA_FP32 is also read by the library (`getenv` in gd4d_self_attn.hip), which keeps its answer for the
    whole process; Python reads it per call.  Set it before the first attention launch and leave it.
  * `read='bench.py'`: documented here, read by bench.py alone (it keeps literal reads of its own; the defaults are the same).

Values.  An empty value counts as unset.  A flag takes `0` / `1` (GD4D_POS_ENCODER also its README names), a choice one of its
list, an integer anything int() parses; every other value raises `_lib.Gd4dError` naming the switch, the value and what is
accepted - a misspelt value never selects a route silently.  GD4D_PREPROJECT stays free-form (`spec`): functional.pipeline_groups
parses it, and anything it does not know means `1`.

The request key.  `SCHEDULE` lists the switches declared `schedule=True` - every switch the code a RequestProgram records reads
(run_single, LateValues, the chain_* descriptors) - and `schedule_key()` is their raw values, part of the program's key.  The
read log holds the declaration to the code: inside `with read_log() as names:` the readers add the name of every switch the current
thread reads while it records (`_lib.recorder() is not None`); RequestProgram keeps that set as `switches_read`, and
tests/test_request_gpu.py asserts that it lies inside SCHEDULE.  Outside the block the log costs one attribute test per read.

This module imports nothing from the package when it is imported (_lib needs it for GD4D_LIB_PATH).
"""
import collections
import os
import threading

Switch = collections.namedtuple('Switch', 'name kind default values meaning schedule read unset')
REGISTRY = {}


def _declare(name, kind, default, meaning, values=None, schedule=False, read='call', unset=None):
    """default: what the reader returns when the switch is unset (None: the caller decides; `unset` says how, in README's words).
    values: a choice's list; for a flag, extra names besides 0 / 1 as {name: bool}."""
    REGISTRY['GD4D_' + name] = Switch('GD4D_' + name, kind, default, values, meaning, schedule, read, unset)


_declare('LIB_PATH', 'path', None, 'alternative libgd4d.so (A/B builds)', read='import', unset='in-tree')
_declare('FUSED_DECODER', 'flag', True, 'inference: the decoder loop on row chains; 0: module by module', schedule=True)
_declare('TRAIN_CHAINS', 'flag', True, 'training: the decoder as one autograd node on row chains; 0: one node per operation')
_declare('PROJECT', 'choice', 'late', 'late: aggregate-then-project; early: value_proj over the pyramid first', ('late', 'early'), schedule=True)
_declare('PREPROJECT', 'spec', 'auto', 'GD4D_PROJECT=early: grouping of the value_proj launches (auto, 0, 1, stream, g2,2,2 ...)')
_declare('PIPELINE_CUS', 'int', None, 'GD4D_PROJECT=early: CUs of the persistent value_proj kernel while overlapped',
         unset='3/4 of the device')
_declare('VALUE_LAYOUT', 'choice', None, 'GD4D_PROJECT=early: layout of the projected values', ('pixel', 'head'), unset='by dtype')
_declare('TRAIN_VALUES', 'choice', 'raw', 'training: raw = no projected value tensor; projected = value_proj over the pyramid',
         ('raw', 'projected'))
_declare('AGG', 'choice', 'sliced', 'sliced: plan + channel-sliced gather; rows: one workgroup per query (B = 1)', ('sliced', 'rows'),
         schedule=True)
_declare('PLAN', 'choice', 'items', 'inference plan form: items (32 B per item) / pairs (what the training kernels read)',
         ('items', 'pairs'), schedule=True)
_declare('POS_ENCODER', 'flag', True, 'position_encoder beside chain B\' through a hand-off (1 = chainb); 0 = dual: no hand-off',
         {'chainb': True, 'dual': False}, schedule=True)
_declare('TRAIN_REG_BESIDE', 'flag', True, 'training: the reg branch beside the next in-projection through a hand-off; 0: at the chain\'s end')
_declare('MHA_FP32', 'flag', False, 'self-attention core with fp32 MFMA products; the library reads it too, ONCE per process', schedule=True)
_declare('QUERY_ORDER', 'flag', True, 'locality order of the queries for the gathers', schedule=True)
_declare('AUX_STREAM', 'flag', True, 'module-by-module path: position_encoder and reg branch on an auxiliary stream')
_declare('COPY_CUS', 'int', None, 'CUs of the persistent slice-planar copy; 0: plain copy', schedule=True, unset='3/4 of the device')
_declare('TORCH_OPS', 'flag', False, 'run the modules that have one through their differentiable torch-op route')
_declare('DIST_BACKEND', 'choice', 'nccl', 'gloo: bench.py --gpus N with all ranks on one GPU', ('nccl', 'gloo'), read='bench.py')
_declare('PREFLIGHT_MB', 'spec', '22,140,330', 'sizes of the all-reduces dist.preflight times before an N > 1 bench', read='bench.py')
_declare('COARSE', 'flag', True, 'inference: the two coarse levels gathered from projected rows; 0: every level raw', schedule=True)
_declare('COARSE_MAX_ROWS', 'int', 65536, 'the coarse levels\' pixel rows up to which GD4D_COARSE applies', schedule=True)
_declare('HEAD_CHAINS', 'flag', True, 'the head\'s box epilogue as two-program row chains; 0: one launch per operation')
_declare('CHAIN_ALL_EXACT', 'flag', False, 'measurement: every chain GEMM on six split-bf16 products; seeds ops.ALL_EXACT', read='import')
_declare('FIRST_PROJ', 'choice', 'main', 'where the first layer\'s coarse projection runs: main stream / side stream', ('main', 'side'),
         schedule=True)
_declare('FILLS_RIDE', 'choice', 'chain', 'training: which launches carry the pyramid gradient\'s record fills', ('chain', 'mha'))
_declare('PE_FRUSTUM', 'flag', True, 'head position embedding: frustum inputs generated in the MLP\'s prologue; 0: written and read')
_declare('PE_FUSED', 'flag', True, 'channels_last_out: both MLPs and the fuse as one kernel; 0: two kernels')
_declare('REQUEST', 'flag', False, 'an eager decoder forward issued by one host call (fused_decoder.RequestProgram)', schedule=True)

SCHEDULE = tuple(s.name for s in REGISTRY.values() if s.schedule)
_FLAG = {'0': False, '1': True}


class _Log(threading.local):
    names = None                    # the set the read log fills in this thread while it is on, else None


_log = _Log()


class read_log:
    """`with switches.read_log() as names:` - `names` collects the switches this thread reads while it records a request program."""

    def __enter__(self):
        self.prev, _log.names = _log.names, set()
        return _log.names

    def __exit__(self, *exc):
        _log.names = self.prev


def _raw(name):
    if _log.names is not None:
        from . import _lib
        if _lib.recorder() is not None:
            _log.names.add(name)
    return os.environ.get(name)


def _refuse(sw, raw, accepted):
    from ._lib import Gd4dError
    raise Gd4dError(f'{sw.name}={raw!r} is not a value of this switch: accepted are {accepted} (unset or empty: {default_text(sw)})')


def flag(name):
    raw = _raw(name)
    if not raw:
        return REGISTRY[name].default
    on = _FLAG.get(raw)
    if on is None:
        sw = REGISTRY[name]
        on = (sw.values or {}).get(raw)
        if on is None:
            _refuse(sw, raw, ', '.join(['0', '1'] + list(sw.values or ())))
    return on


def choice(name):
    raw, sw = _raw(name), REGISTRY[name]
    if not raw:
        return sw.default
    if raw not in sw.values:
        _refuse(sw, raw, ', '.join(sw.values))
    return raw


def integer(name):
    raw = _raw(name)
    if not raw:
        return REGISTRY[name].default
    try:
        return int(raw)
    except ValueError:
        _refuse(REGISTRY[name], raw, 'integers')


def path(name):
    return _raw(name) or REGISTRY[name].default


def spec(name):
    return _raw(name) or REGISTRY[name].default


def schedule_key():
    """The raw values of the SCHEDULE switches, for a request program's key (raw: an unset and an empty one get two programs)."""
    return tuple(map(os.environ.get, SCHEDULE))


def default_text(sw):
    """The default as README.md's table spells it."""
    if sw.default is None:
        return sw.unset
    return {True: '1', False: '0'}[sw.default] if sw.kind == 'flag' else str(sw.default)
