"""The small regularized models of the regularizer tests (CPU, GPU and their worker scripts).

``tiny``: the tiny RPV model of tests/test_clipping_gpu.py::_tiny (16x16xC, conv [4, 8, 8],
fc [16], sigmoid head).  ``odd``: the "odd" model of tests/test_hip_model.py::_build (layer sizes
that are no multiples of 4, two hidden denses, softmax head).  ``reg=True`` puts l1_l2 on every
kernel and l2 on one bias (so range borders fall anywhere); ``reg=False`` builds the same model
with no regularizer argument at all."""
from cori_intml_examples_amd import regularizers
from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model

L1, L2, BIAS_L2 = 1e-3, 1e-2, 5e-2


def _kw(reg, bias=False):
    if not reg:
        return {}
    kw = {"kernel_regularizer": regularizers.l1_l2(L1, L2)}
    if bias:
        kw["bias_regularizer"] = regularizers.l2(BIAS_L2)
    return kw


def tiny(opt, device="cpu", channels=3, drop=0.0, reg=True, dp=False):
    inp = Input(shape=(16, 16, channels))
    h = inp
    for i, c in enumerate((4, 8, 8)):
        h = Conv2D(c, kernel_size=(3, 3), activation="relu", padding="same", **_kw(reg, bias=i == 1))(h)
        h = MaxPooling2D(pool_size=(2, 2))(h)
    h = Dropout(drop)(h)
    h = Flatten()(h)
    h = Dense(16, activation="relu", **_kw(reg))(h)
    h = Dropout(drop)(h)
    out = Dense(1, activation="sigmoid", **_kw(reg))(h)
    m = Model(inputs=inp, outputs=out, name="RPVClassifier", device=device)
    m.compile(optimizer=_dist(opt, dp), loss="binary_crossentropy", metrics=["accuracy"])
    return m


def odd(opt, device="cpu", drop=0.0, reg=True):
    inp = Input(shape=(19, 17, 2))
    h = Conv2D(5, (3, 3), activation="relu", padding="same", **_kw(reg))(inp)
    h = MaxPooling2D((2, 2))(h)
    h = Conv2D(12, (3, 3), activation="relu", **_kw(reg, bias=True))(h)
    h = MaxPooling2D((2, 2))(h)
    h = Flatten()(h)
    h = Dense(20, activation="relu", **_kw(reg))(h)
    h = Dropout(drop)(h)
    h = Dense(9, activation="relu", **_kw(reg))(h)
    out = Dense(3, activation="softmax", **_kw(reg))(h)
    m = Model(inp, out, device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


def _dist(opt, dp):
    if not dp:
        return opt
    from cori_intml_examples_amd.parallel import hvd
    return hvd.DistributedOptimizer(opt)
