"""CPU: the Whisper training path's new entry points are declared, bound with matching argument counts, and built free of packed-f32 instructions."""
import os
import subprocess

import pytest

from test_abi_cpu import _header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_attention_qkv_bwd_fused",)


@pytest.fixture(scope="module")
def built():
    from huggingface_asr_amd.csrc import build as B
    return B.build()


def test_fused_attention_backward_is_declared_and_bound(built):
    from huggingface_asr_amd import _lib
    decl = _header_functions()
    h = _lib.lib()
    for n in NEW:
        assert n in decl and hasattr(h, n)
        assert len(_lib.SIGNATURES[n]) == decl[n]


def test_fused_attention_backward_object_has_no_packed_f32(built):
    obj = os.path.join(ROOT, "huggingface_asr_amd", "csrc", "build", "attn_bwd_fused.o")
    tool = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(obj) or not os.path.exists(tool):
        pytest.skip("no object file / no llvm-objdump here")
    from huggingface_asr_amd.csrc import build as B
    B.check_no_packed_f32([obj])


def test_training_calls_no_longer_route_to_transformers_on_device_tensors():
    """the routing decision itself (no GPU needed): a training call with dropout 0 takes the HIP autograd path; dropout > 0 is handed to transformers"""
    import inspect
    from huggingface_asr_amd import whisper
    src = inspect.getsource(whisper.hip_whisper_encoder_forward)
    assert "_encoder_train_forward" in src and '"training mode"' not in src
    assert issubclass(whisper._WhisperEncoderFn, __import__("torch").autograd.Function)
