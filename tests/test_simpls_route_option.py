"""The ``simpls_global`` route switch is a plsx_set_option key (no GPU needed: the keys come from libplsx.so)."""
from pypyls_amd import engine


def test_simpls_global_is_an_option_key():
    assert 'simpls_global' in engine.option_names()
    assert engine.options_from_env({'PLSX_SIMPLS_GLOBAL': '1'}) == {'options': {'simpls_global': 1}}
