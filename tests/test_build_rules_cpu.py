"""build_lib.RESOURCE_RULES / _check_usage: the per-source rules on the
compiler's kernel-resource-usage remarks, fed remark text made here."""
import pytest

from quicfuscate_amd import build_lib


def _remarks(funcs):
    """Remark text in hipcc's form for {function name: scratch bytes per lane}."""
    out = []
    for name, scratch in funcs.items():
        pre = "src.hip:1:1: remark: "
        out += [f"{pre}Function Name: {name} [-Rpass-analysis=kernel-resource-usage]",
                f"{pre}    VGPRs: 24 [-Rpass-analysis=kernel-resource-usage]",
                f"{pre}    ScratchSize [bytes/lane]: {scratch} [-Rpass-analysis=kernel-resource-usage]",
                f"{pre}    Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]"]
    return "\n".join(out) + "\n"


def _clean(src):
    """A passing set of functions for a source: one per name of its rule, spread
    over `count` instantiations, plus one function the rule does not name."""
    rule = build_lib.RESOURCE_RULES[src]
    n = rule.count if rule.count is not None else len(rule.names)
    funcs = {f"_ZN2qf{rule.names[i % len(rule.names)]}ILi{i}EEEvNS_4ArgsE": 0 for i in range(n)}
    funcs["_ZN2qf7k_otherENS_4ArgsE"] = 0
    return funcs


def test_remark_sources_follow_the_table():
    assert set(build_lib.REMARK_SOURCES) == set(build_lib.RESOURCE_RULES) | {"qf_gf16_bs.hip"}
    assert set(build_lib.REMARK_SOURCES) <= set(build_lib.SOURCES)


@pytest.mark.parametrize("src", sorted(build_lib.RESOURCE_RULES))
def test_clean_remarks_pass(src):
    funcs = _clean(src)
    usage = build_lib._check_usage(src, _remarks(funcs))
    assert set(usage) == set(funcs)
    assert all(u == {"VGPRs": 24, "ScratchSize": 0, "Occupancy": 8} for u in usage.values())


@pytest.mark.parametrize("src", sorted(s for s, r in build_lib.RESOURCE_RULES.items() if r.count is not None))
def test_missing_instantiation_raises(src):
    funcs = _clean(src)
    del funcs[next(iter(funcs))]
    with pytest.raises(RuntimeError):
        build_lib._check_usage(src, _remarks(funcs))


@pytest.mark.parametrize("src", sorted(build_lib.RESOURCE_RULES))
def test_scratch_on_a_checked_name_raises(src):
    funcs = _clean(src)
    funcs[next(iter(funcs))] = 16
    with pytest.raises(RuntimeError):
        build_lib._check_usage(src, _remarks(funcs))


def test_scratch_on_an_unchecked_name():
    """qf_kernels.hip checks only the k_combine_* kernels; qf_recode.hip and
    qf_rank.hip every function of the file."""
    for src, raises in (("qf_kernels.hip", False), ("qf_relay.hip", False), ("qf_recode.hip", True),
                        ("qf_rank.hip", True)):
        funcs = _clean(src)
        funcs["_ZN2qf7k_otherENS_4ArgsE"] = 16
        if raises:
            with pytest.raises(RuntimeError):
                build_lib._check_usage(src, _remarks(funcs))
        else:
            assert build_lib._check_usage(src, _remarks(funcs))["_ZN2qf7k_otherENS_4ArgsE"]["ScratchSize"] == 16
