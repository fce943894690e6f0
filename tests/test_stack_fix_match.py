"""The host's choice of the conv-stack instance with the whole geometry fixed at compile time
(K.conv_stack_fixed, the query launch_conv_stack_fwd's own decision goes through): true for the
RPV stack at two row bands at any batch, false as soon as one geometry field of the args, one LDS
offset, one entry of the band table, a compiled-in switch or a spec / fix / diagnostics setting
differs.  No GPU: the query is host arithmetic on the argument struct; the device pointers are
stand-in non-null addresses that nothing reads.

The args are written out from scripts/plan_dump.py's dump of the RPV bench model's B = 128
training plan (the `stack` of conv_stack_fwd) and from hip_geometry._stack_rows / _stack_layout at
two bands, not read from the signature under test."""
import pytest

from cori_intml_examples_amd.ops.hip import kernels

K = kernels()          # the project's loader: a missing or broken extension is an error, not a skip

PTR = 1 << 20
SAME = dict(KH=3, KW=3, pad_t=1, pad_l=1, pool=1, relu=1)
LAYERS = [
    dict(H=64, W=64, Cs_in=4, Ho=64, Wo=64, Cout=16, Cs_out=16, KS=2, NT=1, Hp=32, Wp=32, w_lds=0, xpix=4, xrow=74),
    dict(H=32, W=32, Cs_in=16, Ho=32, Wo=32, Cout=32, Cs_out=32, KS=5, NT=2, Hp=16, Wp=16, w_lds=1024, xpix=16,
         xrow=36),
    dict(H=16, W=16, Cs_in=32, Ho=16, Wo=16, Cout=64, Cs_out=64, KS=9, NT=4, Hp=8, Wp=8, w_lds=6144, xpix=48,
         xrow=20),
]
ROWS = [[(0, 38, 0, 16, -1, 40), (26, 64, 16, 32, 25, 40)],
        [(0, 18, 0, 8, -1, 20), (14, 32, 8, 16, 13, 20)],
        [(0, 8, 0, 4, -1, 10), (8, 16, 4, 8, 7, 10)]]
ARGS = dict(n=3, splits=2, off_bias=1312, off_w=2336, off_codes=98208, off_codes2=107936, lds_bytes=117664, k16=1,
            wt=1, spec=2)
BUFS = (51488, 75168)


def _args(bs=128, layer_edit=None, rows_edit=None, bufs=BUFS, **edit):
    a = K.ConvStackArgs()
    for k, v in {**ARGS, "B": bs, "seed": 7, **edit}.items():
        setattr(a, k, v)
    a.x = a.st = a.srcidx = PTR
    a.set_buf_offsets(*bufs)
    for l, fields in enumerate(LAYERS):
        L = K.StackLayer()
        for k, v in dict(fields, **SAME).items():
            setattr(L, k, v)
        if layer_edit and layer_edit[0] == l:
            setattr(L, layer_edit[1], layer_edit[2])
        L.wpk = L.bias = L.out = L.code = PTR
        L.drop_thr, L.drop_scale, L.stream_id = 0x33333333, 1.25, l + 1
        a.set_layer(l, L)
        for sp in range(2):
            r = list(ROWS[l][sp])
            if rows_edit and rows_edit[:2] == (l, sp):
                r[rows_edit[2]] += rows_edit[3]
            a.set_rows(l, sp, *r)
    return a


@pytest.mark.parametrize("bs", [1, 3, 128, 200])
def test_signature_args_take_the_fixed_kernel(bs):
    a = _args(bs)
    assert a.fix == 1                                          # the struct's default
    assert K.conv_stack_variant(a) == 1                        # the 16-wave instance it replaces
    assert K.conv_stack_fixed(a)


def test_runtime_fields_do_not_matter():
    """Hyperparameters and step switches stay run-time: one instance serves training and
    evaluation, any dropout rate, a model without biases or codes."""
    a = _args(from_data=1, training=1, step_inc=1, seed=12345)
    assert K.conv_stack_fixed(a)
    for l in range(3):
        L = K.StackLayer()
        for k, v in dict(LAYERS[l], **SAME).items():
            setattr(L, k, v)
        L.wpk = L.out = PTR                                    # no bias, no codes, no dropout
        a.set_layer(l, L)
    assert K.conv_stack_fixed(a)


def test_any_setting_declines():
    assert not K.conv_stack_fixed(_args(fix=0))                # stack_fix=0
    assert not K.conv_stack_fixed(_args(spec=0))               # stack_spec=0: the generic kernel
    assert not K.conv_stack_fixed(_args(spec=1))               # the 12-wave instances were asked for
    assert not K.conv_stack_fixed(_args(dbg=128))              # a diagnostics launch
    assert not K.conv_stack_fixed(_args(ts=PTR))               # a stamp launch
    assert not K.conv_stack_fixed(_args(k16=0))
    assert not K.conv_stack_fixed(_args(wt=0))
    assert not K.conv_stack_fixed(_args(B=0))


@pytest.mark.parametrize("field", ["n", "splits", "off_bias", "off_w", "off_codes", "off_codes2", "lds_bytes"])
def test_any_layout_field_declines(field):
    assert not K.conv_stack_fixed(_args(**{field: ARGS[field] + (1 if field in ("n", "splits") else 16)}))


def test_buffer_offsets_decline():
    assert not K.conv_stack_fixed(_args(bufs=(BUFS[0] + 16, BUFS[1])))
    assert not K.conv_stack_fixed(_args(bufs=(BUFS[0], BUFS[1] + 16)))


GEO = ["H", "W", "Cs_in", "Ho", "Wo", "Cout", "Cs_out", "KH", "KW", "pad_t", "pad_l", "KS", "NT", "pool", "relu", "Hp",
       "Wp", "w_lds", "xpix", "xrow"]


@pytest.mark.parametrize("l", [0, 1, 2])
@pytest.mark.parametrize("field", GEO)
def test_any_layer_field_declines(l, field):
    base = dict(LAYERS[l], **SAME)[field]
    other = 0 if field in ("pool", "relu") else base + 1
    assert not K.conv_stack_fixed(_args(layer_edit=(l, field, other))), (l, field)


@pytest.mark.parametrize("l", [0, 1, 2])
@pytest.mark.parametrize("sp", [0, 1])
@pytest.mark.parametrize("i", range(6))
def test_any_band_row_declines(l, sp, i):
    assert not K.conv_stack_fixed(_args(rows_edit=(l, sp, i, 2))), (l, sp, i)


def test_missing_pointers_decline():
    a = _args()
    a.x = 0
    assert not K.conv_stack_fixed(a)
    for f in ("wpk", "out"):
        a = _args()
        L = K.StackLayer()
        for k, v in dict(LAYERS[1], **SAME).items():
            setattr(L, k, v)
        L.wpk = L.out = L.bias = L.code = PTR
        setattr(L, f, 0)
        a.set_layer(1, L)
        assert not K.conv_stack_fixed(a), f
