"""d3p_amd/csrc/d3p_colreduce.h, host side: what the column reducers share is defined once (the float32 order-key map, the opt-in to
dynamic LDS, the 144 KiB figure), the header is a build dependency, and the training translation units stay clear of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "d3p_amd", "csrc")
HEADER = "d3p_colreduce.h"
USERS = ("d3p_psis.hip", "d3p_quantiles.hip", "d3p_hpdi.hip", "d3p_grad_norms.hip", "d3p_gmm_density.hip", "d3p_predict_gmm.hip")
TRAINING = ("d3p_dpvi.hip", "d3p_stages.hip", "d3p_gmm.hip", "d3p_vae.hip", "d3p_gemm.hip", "d3p_rng.hip", "d3p_host.h", "d3p_device.h")


def _texts():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            out[name] = f.read()
    return out


def _files_with(texts, needle):
    return sorted(name for name, text in texts.items() if needle in text)


def test_one_definition_of_the_order_key_and_the_lds_opt_in():
    texts = _texts()
    assert sum(text.count("? 0xffffffffu : 0x80000000u") for text in texts.values()) == 1   # one float32 key map
    assert _files_with(texts, "? 0xffffffffu : 0x80000000u") == [HEADER]
    assert _files_with(texts, "hipFuncSetAttribute") == [HEADER, "d3p_dpvi.hip", "d3p_logreg_particles.h"]
    assert _files_with(texts, "147456") == [HEADER]                                          # one 144 KiB figure


def test_the_header_is_a_build_dependency_of_its_users_only():
    import d3p_amd._lib as L
    assert os.path.join(CSRC, HEADER) in L._DEPS
    texts = _texts()
    include = re.compile(r'#include\s+"%s"' % re.escape(HEADER))
    assert sorted(name for name, text in texts.items() if include.search(text)) == sorted(USERS)
    training = [name for name in texts if name in TRAINING or name.startswith("d3p_logreg_")]
    assert len(training) == len(TRAINING) + 5                                                # the five d3p_logreg_*.h
    for name in training:
        assert HEADER not in texts[name], name
