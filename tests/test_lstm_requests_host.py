"""Every refusal of the eight LSTM entry points (bore_lstm_X / bore_lstm_stream_X) without a GPU: the return code and
the full text of bore_last_error(), case by case, in an order that pins the order of the checks -- n_models, T, the
flavour's layout and bounds, pointers, the rest, and the "nothing to do" returns where they sit.  Every verdict is
reached before the first HIP call, so the data pointers here are a few host bytes that nobody reads.

The expected texts were recorded from the library as it was BEFORE the two flavours shared their request checks
(loaded through BORE_LIB_PATH), not from the code under test.  The flavours differ in the prefix of a message
({who}: the entry point, {fl}: the flavour) and in their bounds; everything else is one table per entry kind."""
import ctypes

import pytest

OK, E_INVALID, E_UNSUPPORTED = 0, -1, -2
FLAVOURS = {"lds": ("bore_lstm_", "lstm_", "lstm"), "stream": ("bore_lstm_stream_", "lstm_stream_", "lstm_stream")}
NULL_DESC = "lstm: null descriptor"
UNTOUCHED = NULL_DESC   # what a call that returns 0 leaves in bore_last_error(): the text that was there before


@pytest.fixture(scope="module")
def built():
    import os
    from bore_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    return _lib.lib()


_BYTES = ctypes.create_string_buffer(64)
PTR = ctypes.cast(_BYTES, ctypes.c_void_p)


def _desc(D=3, L=2, H=5, act=2, output_dim=1):
    from bore_amd import _lib
    d = _lib.LstmDesc()      # (not make_lstm_desc: it refuses five layers itself)
    d.input_dim, d.n_layers, d.units, d.act, d.output_dim = D, L, H, act, output_dim
    return d


# the descriptor and the bounds: (case, descriptor fields or None, T, code, text), shared by the four entry kinds.
# Each case ALSO passes a null theta: the descriptor, T and the bounds are reported ahead of the pointers.
DESC_CASES = [
    ("null descriptor", None, 3, E_INVALID, NULL_DESC),
    ("T = 0", {}, 0, E_INVALID, "{who}: need at least one step (got 0)"),
    ("T = 0 ahead of a null descriptor", None, 0, E_INVALID, "{who}: need at least one step (got 0)"),
    ("T = 17", {}, 17, E_UNSUPPORTED, "{fl}: 17 steps > 16 (BORE_LSTM_MAX_STEPS)"),
    ("output_dim = 2", dict(output_dim=2), 3, E_UNSUPPORTED, "lstm: output_dim must be 1 (the BORE classifier), got 2"),
    ("zero units", dict(H=0), 3, E_INVALID, "lstm: input_dim, n_layers and units must be positive (got 3, 2, 0)"),
    ("unknown activation", dict(act=9), 3, E_INVALID, "lstm: unknown activation 9"),
    ("five layers", dict(L=5), 3, E_UNSUPPORTED, "{fl}: n_layers 5 > 4 (BORE_LSTM_MAX_LAYERS)"),
]
BOUND_CASES = {
    "lds": [
        ("65 inputs", dict(D=65), 3, E_UNSUPPORTED, "lstm: input_dim 65 > 64 (BORE_LSTM_MAX_INPUT)"),
        ("65 units", dict(H=65), 3, E_UNSUPPORTED, "lstm: units 65 > 64 (BORE_LSTM_MAX_UNITS)"),
        ("the LDS of one CU", dict(D=2, L=3, H=32), 5, E_UNSUPPORTED,
         "lstm: 2 inputs, 3 layers of 32 units over 5 steps need 182032 B of LDS per workgroup (> 163840): parameters "
         "(21153 floats) and one tile of state must fit one CU"),
    ],
    "stream": [
        ("513 inputs", dict(D=513), 3, E_UNSUPPORTED, "lstm_stream: input_dim 513 > 512 (BORE_LSTM_STREAM_MAX_INPUT)"),
        ("129 units", dict(H=129), 3, E_UNSUPPORTED, "lstm_stream: units 129 > 128 (BORE_LSTM_STREAM_MAX_UNITS)"),
    ],
}

# per entry kind: the arguments behind (desc, n_models) of a call that nothing is wrong with, by name, and the cases
# (case, overrides, code, text[, the one flavour the case holds for]) in the order of the checks
FORWARD = dict(theta=PTR, X=PTR, n_rows=1, T=3, many_to_many=1, mask_value=-1.0, out=PTR)
FORWARD_CASES = [
    ("n_models = 0", dict(n_models=0, T=0, theta=None), E_INVALID, "{who}: n_models must be >= 1 (got 0)"),
    ("theta = NULL", dict(theta=None, n_rows=-1), E_INVALID, "{who}: null pointer"),
    ("X = NULL", dict(X=None), E_INVALID, "{who}: null pointer"),
    ("out = NULL", dict(out=None), E_INVALID, "{who}: null pointer"),
    ("n_rows = -1", dict(n_rows=-1), E_INVALID, "{who}: n_rows < 0"),
    ("n_rows = 0", dict(n_rows=0), OK, UNTOUCHED),
]
VALUE_GRAD = dict(theta=PTR, X=PTR, n_rows=1, T=3, transform=1, negate=1, val=PTR, grad=PTR)
VALUE_GRAD_CASES = [
    ("n_models = 0", dict(n_models=0, T=0, theta=None), E_INVALID, "{who}: n_models must be >= 1 (got 0)"),
    ("theta = NULL", dict(theta=None, transform=7), E_INVALID, "{who}: null pointer"),
    ("X = NULL", dict(X=None), E_INVALID, "{who}: null pointer"),
    ("val = NULL", dict(val=None), E_INVALID, "{who}: null pointer"),
    ("grad = NULL", dict(grad=None), E_INVALID, "{who}: null pointer"),
    ("unknown transform", dict(transform=7, n_rows=-1), E_INVALID, "{who}: unknown transform 7"),
    ("n_rows = -1", dict(n_rows=-1), E_INVALID, "{who}: n_rows < 0"),
    ("n_rows = 0", dict(n_rows=0), OK, UNTOUCHED),
]
FIT = dict(theta=PTR, adam_m=PTR, adam_v=PTR, adam_t=PTR, X=PTR, y=PTR, N=70, T=3, mask_value=-1.0, epochs=3,
           batch_size=32, perm=PTR, adam=PTR, epoch_loss=None)
FIT_CASES = [
    ("n_models = 0", dict(n_models=0, T=0, theta=None), E_INVALID, "{who}: n_models must be >= 1 (got 0)"),
] + [
    (name + " = NULL", {name: None, "N": 0}, E_INVALID, "{who}: null pointer")
    for name in ("theta", "adam_m", "adam_v", "adam_t", "X", "y", "adam")
] + [
    ("N = 0", dict(N=0, batch_size=0), E_INVALID, "{who}: N must be >= 1 and epochs >= 0"),
    ("epochs = -1", dict(epochs=-1, batch_size=65), E_INVALID, "{who}: N must be >= 1 and epochs >= 0"),
    ("batch_size = 0", dict(batch_size=0, epochs=0), E_INVALID, "{who}: batch_size must be >= 1"),
    ("batch_size = 65", dict(batch_size=65, epochs=0), E_UNSUPPORTED,
     "{who}: batch_size 65 > 64 (one tile of sequences per Adam step)"),
    ("epochs = 0", dict(epochs=0, perm=None, N=2 ** 31), OK, UNTOUCHED),
    ("perm = NULL", dict(perm=None, N=2 ** 31), E_INVALID, "{who}: explicit per-epoch permutations are required"),
    ("N = 2^31", dict(N=2 ** 31), E_UNSUPPORTED, "{who}: N > 2^31 - 1"),
]
EVALUATE = dict(theta=PTR, X=PTR, y=PTR, N=70, T=3, mask_value=-1.0, loss=PTR, acc=PTR)
EVALUATE_CASES = [
    ("n_models = 0", dict(n_models=0, T=0, theta=None), E_INVALID, "{who}: n_models must be >= 1 (got 0)"),
] + [
    (name + " = NULL", {name: None, "N": 0}, E_INVALID, "{who}: null pointer") for name in ("theta", "X", "y", "loss", "acc")
] + [
    ("N = 0", dict(N=0), E_INVALID, "{who}: N < 1"),
    # (the LDS flavour has no such bound: a workgroup walks its model's rows by a 64-bit index)
    ("N = 2^31", dict(N=2 ** 31), E_UNSUPPORTED, "{who}: N > 2^31 - 1", "stream"),
]
KINDS = {"forward": (FORWARD, FORWARD_CASES), "value_and_input_grad": (VALUE_GRAD, VALUE_GRAD_CASES),
         "fit": (FIT, FIT_CASES), "evaluate": (EVALUATE, EVALUATE_CASES)}


def _call(lib, flavour, kind, desc, n_models, args):
    from bore_amd import _lib
    symbol, who, fl = FLAVOURS[flavour]
    assert lib.bore_lstm_forward(None, 1, None, None, 1, 3, 0, 0.0, None, None) == E_INVALID    # leaves UNTOUCHED behind
    vals = dict(args)
    if kind == "fit" and vals["adam"] is not None:
        cfg = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-7)
        vals["adam"] = ctypes.byref(cfg)
    rc = getattr(lib, symbol + kind)(None if desc is None else ctypes.byref(desc), n_models, *vals.values(), None)
    return rc, lib.bore_last_error().decode(), dict(who=who + kind, fl=fl)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_descriptor_steps_and_bounds_are_refused_ahead_of_the_pointers(built, flavour, kind):
    for case, fields, T, code, text in DESC_CASES + BOUND_CASES[flavour]:
        args = dict(KINDS[kind][0], T=T, theta=None)
        rc, msg, names = _call(built, flavour, kind, None if fields is None else _desc(**fields), 1, args)
        assert (rc, msg) == (code, text.format(**names)), (case, rc, msg)


REQUEST_CASES = [(f, k, c) for f in FLAVOURS for k in KINDS for c in KINDS[k][1] if len(c) == 4 or c[4] == f]


@pytest.mark.parametrize("flavour,kind,case", REQUEST_CASES, ids=["%s %s: %s" % (f, k, c[0]) for f, k, c in REQUEST_CASES])
def test_request_refusals_in_the_order_of_the_checks(built, flavour, kind, case):
    name, overrides, code, text = case[:4]
    overrides = dict(overrides)
    n_models = overrides.pop("n_models", 1)
    rc, msg, names = _call(built, flavour, kind, _desc(), n_models, dict(KINDS[kind][0], **overrides))
    assert (rc, msg) == (code, text.format(**names)), (name, rc, msg)
