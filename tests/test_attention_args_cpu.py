"""CPU: the LDS-staged attention entries refuse every single-defect call of tests/attention_arg_cases.py with the recorded code — MI_ERR_ARG before MI_ERR_UNSUPPORTED —
before anything is launched: the addresses are fake and there is no GPU here."""
import pytest

import attention_arg_cases as A


@pytest.fixture(scope="module")
def lib():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    B.build()
    return _lib.lib()


def test_no_case_expects_a_launch():
    assert len(A.CASES) >= 60 and {e for e, *_ in A.CASES} == set(A.PARAMS)
    for entry, what, args, code in A.CASES:
        assert code in (A.ARG, A.UNSUPPORTED) and code != 0, (entry, what)
        assert args != A.BASES[entry], (entry, what)
    assert any(code == A.UNSUPPORTED for *_, code in A.CASES)


def test_argument_order_matches_the_binding():
    from huggingface_asr_amd import _lib
    for entry, names in A.PARAMS.items():
        sig = _lib.SIGNATURES[entry]
        assert len(sig) == len(names) + 1                                              # + the stream
        assert [n for n, t in zip(names, sig) if t is _lib.vp] == [n for n in names if n in A.POINTERS], entry


@pytest.mark.parametrize("entry,what,args,code", A.CASES, ids=[f"{e[len('mi_attention_'):]}: {w}" for e, w, _, _ in A.CASES])
def test_refused(lib, entry, what, args, code):
    rc = getattr(lib, entry)(*[args[n] for n in A.PARAMS[entry]], None)
    assert rc == code, f"{entry}, {what}: returned {rc}, recorded {code}"
