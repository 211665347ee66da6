"""The streamed flavour's host side (no GPU): which networks `bore_mlp_streamed` says run with
their parameters in global memory, its bounds, and the C-ABI declaration."""
import re

import pytest

from bore_amd import _lib, ops


def desc(D, units, compute="float32"):
    return _lib.make_desc(D, units, ["relu"] * (len(units) - 1) + ["linear"], compute=compute)


@pytest.mark.parametrize("D,units,mask", [
    (8, [256, 256, 1], 7),          # 68 353 parameters: ~265 KB in the LDS layout
    (16, [128, 128, 128, 1], 7),    # ClassifierSuggester(num_units=128, num_layers=2) on 16 inputs
    (2, [16, 16, 1], 0),
    (32, [128, 128, 1], 0),         # the widest network the LDS flavours take
])
def test_which_networks_stream(D, units, mask):
    assert ops.mlp_streamed(desc(D, units)) == mask


def test_bounds_are_named():
    with pytest.raises(_lib.UnsupportedError, match="BORE_STREAM_MAX_UNITS"):
        ops.mlp_streamed(desc(8, [513, 513, 1]))
    assert _lib.STREAM_MAX_UNITS == 512
    assert ops.mlp_streamed(desc(8, [512, 512, 1])) == 7
    assert ops.mlp_streamed(desc(512, [512] * 7 + [1])) == 7      # the largest network of the flavour


def test_bfloat16_is_never_streamed():
    assert ops.mlp_streamed(desc(32, [128, 128, 1], compute="bfloat16")) == 0
    assert ops.mlp_streamed(desc(8, [256, 256, 1], compute="bfloat16")) == 0


def test_the_query_ignores_the_forcing_switch(monkeypatch):
    monkeypatch.setenv("BORE_STREAM", "1")
    assert ops.mlp_streamed(desc(2, [16, 16, 1])) == 0
    assert ops.mlp_streamed(desc(8, [256, 256, 1])) == 7


def test_symbol_is_exported_and_declared():
    assert "bore_mlp_streamed" in _lib.EXPORTS
    with open(_lib.HEADER) as f:
        header = f.read()
    assert re.search(r"\bint\s+bore_mlp_streamed\s*\(\s*const\s+bore_mlp_desc\s*\*\s*desc\s*\)\s*;", header)
    assert re.search(r"#define\s+BORE_STREAM_MAX_UNITS\s+512\b", header)
    assert _lib.abi_version_of_header() == 12                     # additive
    assert hasattr(_lib.lib(), "bore_mlp_streamed")
