"""d3p_amd/csrc/d3p_row_sums.h, host side: what the per-draw reductions over rows share is defined once (the strip function, the strip
merge, the workspace check), the link and the obs-key staging of their kernels are defined once beside the tile and the outcome rules,
the header is a build dependency of its four users, and the training translation units stay clear of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "d3p_amd", "csrc")
HEADER = "d3p_row_sums.h"
USERS = ("d3p_draw_sums.hip", "d3p_rep_stats.hip", "d3p_discrepancy.hip", "d3p_gmm_density.hip")
TRAINING = ("d3p_dpvi.hip", "d3p_stages.hip", "d3p_gmm.hip", "d3p_vae.hip", "d3p_gemm.hip", "d3p_rng.hip")
# strip rules of their own, NOT part of this family: chunks of 256 rows with a cap per kernel; strips of a vector of norms
OTHER_STRIP_RULES = {"d3p_model_weights.hip": "*strips = *chunks ? cdiv(*chunks, *per) : 0;", "d3p_grad_norms.hip": "static uint32_t np_strips(uint64_t n)"}


def _texts():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            out[name] = f.read()
    return out


def _files_with(texts, needle):
    return sorted(name for name, text in texts.items() if needle in text)


def _count(texts, needle):
    return sum(text.count(needle) for text in texts.values())


def test_one_strip_function_one_merge_and_one_workspace_check():
    texts = _texts()
    assert _files_with(texts, "cdiv(*tiles,") == [HEADER] and _count(texts, "cdiv(*tiles,") == 2        # per and strips, once each
    assert _files_with(texts, "? cdiv(*") == sorted([HEADER, "d3p_model_weights.hip"])                  # no third copy of the shape
    for name, needle in OTHER_STRIP_RULES.items():
        assert needle in texts[name] and HEADER not in texts[name], name
    assert _count(texts, "#define D3P_ROW_SUMS_MAX_STRIPS 512") == 1
    for gone in ("D3P_DRAW_SUMS_MAX_STRIPS", "D3P_REP_MAX_STRIPS", "D3P_DISC_MAX_STRIPS", "draw_sums_strips", "rep_strips", "disc_strips",
                 "gd_strips", "k_draw_sums_merge", "k_gmm_draw_sums_merge", "k_rep_stats_merge", "k_discrepancy_merge", "disc_mean",
                 "rep_workspace_check"):
        assert _files_with(texts, gone) == [], gone
    assert len(re.findall(r"__global__[^\n]*\bk_strip_merge\(", texts[HEADER])) == 1
    assert _files_with(texts, "double rep_min(") == [HEADER] and _files_with(texts, "double rep_max(") == [HEADER]
    assert _files_with(texts, ": the workspace must be") == [HEADER]                                    # one wording, one order
    assert _count(texts, "row_workspace_check(what, ") == 5 and _count(texts, "row_workspace_check(") == 6   # five entries, one definition
    merges = {name: sorted(set(re.findall(r"strip_merge<([^>]*)>\(what", text))) for name, text in texts.items() if name in USERS}
    assert merges == {"d3p_draw_sums.hip": ["1, -1, -1"], "d3p_gmm_density.hip": ["1, -1, -1"], "d3p_rep_stats.hip": ["D3P_REP_STATS, 2, 3"],
                      "d3p_discrepancy.hip": ["D3P_DISC_SUMS, -1, -1"]}
    assert "#define D3P_REP_STATS 5" in texts["d3p_rep_stats.hip"] and "#define D3P_DISC_SUMS 6" in texts["d3p_discrepancy.hip"]


def test_one_sigmoid_one_key_staging_and_one_outcome_choice():
    texts = _texts()
    assert _count(texts, "1.0f / den") == 1 and _files_with(texts, "1.0f / den") == ["d3p_glm_tile.h"]
    assert _count(texts, "threefry2x32(o0, o1, 0u, 0u") == 1 and _files_with(texts, "threefry2x32(o0, o1, 0u, 0u") == ["d3p_outcome.h"]
    outcome = texts["d3p_outcome.h"]
    assert len(re.findall(r"\bauto glm_outcome\(", outcome)) == 1 and _count(texts, "auto glm_outcome(") == 1
    body = outcome[outcome.index("auto glm_outcome("):]
    for rule in ("normal_site_value(", "poisson_draw(", "bernoulli_draw(", "sigmoid_probs("):
        assert rule in body, rule                                                                       # on top of the one rule each
    for name in ("d3p_rep_stats.hip", "d3p_discrepancy.hip"):
        assert "glm_outcome<FAMILY>(" in texts[name] and "stage_obs_keys<FAMILY>(" in texts[name], name
    for name in ("d3p_moments.hip", "d3p_quantiles.hip", "d3p_discrepancy.hip"):
        assert "glm_mean<FAMILY>(" in texts[name] and "expf(-fabsf(" not in texts[name], name
    assert "sigmoid_pair(" in texts["d3p_moments.hip"]


def test_the_header_is_a_build_dependency_of_its_users_only():
    import d3p_amd._lib as L
    assert os.path.join(CSRC, HEADER) in L._DEPS
    texts = _texts()
    include = re.compile(r'#include\s+"%s"' % re.escape(HEADER))
    assert sorted(name for name, text in texts.items() if include.search(text)) == sorted(USERS)
    training = [name for name in texts if name in TRAINING or name.startswith("d3p_logreg_")]
    assert len(training) == len(TRAINING) + 5                                                           # the five d3p_logreg_*.h
    for name in training:
        assert HEADER not in texts[name], name
