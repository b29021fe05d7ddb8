"""The ``crosscov_sparse`` test hook is a plsx_set_option key (no GPU needed: the keys come from libplsx.so)."""
from pypyls_amd import engine


def test_crosscov_sparse_is_an_option_key():
    names = engine.option_names()
    assert 'crosscov_sparse' in names
    assert len(names) == len(set(names))
    assert engine.options_from_env({'PLSX_CROSSCOV_SPARSE': '1'}) == {'options': {'crosscov_sparse': 1}}
