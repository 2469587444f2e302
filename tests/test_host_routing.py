"""CPU: the rule that picks the layer loop of an eval forward (CaptionBertEncoder.serves_deferred_ln) at the SHIPPED
threshold -- the test session runs with VT_DEFERRED_LN_MIN_ROWS=0 (tests/conftest.py), a user with the default.  Constructor
only: no forward, no GPU."""
import pytest


def _encoder(width, **overrides):
    from visitron_amd.config import BertConfig, mini_config
    from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT, CaptionBertEncoder

    cfg = mini_config(**overrides) if width == 128 else BertConfig(num_hidden_layers=2, **overrides)
    assert cfg.hidden_size == width
    enc = CaptionBertEncoder(cfg)
    enc.deferred_ln_min_rows = DEFERRED_LN_MIN_ROWS_DEFAULT
    return enc


# token rows of a padded forward -> the deferred-LayerNorm loop serves it.  456 = configs[0] (2 x 228), 1 534 = the shipped
# pretrain batch (2 x 767), 2 736 / 2 964 = 12 / 13 sequences of 228 (the last batch below and the first above), 4 088 = the
# rollout's 8 x 511; None = a caller that does not say (the rule then does not look at the row count)
ROWS = [(456, False), (1534, False), (2736, False), (2799, False), (2800, True), (2964, True), (4088, True), (None, True)]


@pytest.mark.parametrize("width", [128, 768])
def test_routing_table_at_the_shipped_threshold(width):
    from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT

    assert DEFERRED_LN_MIN_ROWS_DEFAULT == 2800
    enc = _encoder(width)
    for rows, deferred in ROWS:
        assert enc.serves_deferred_ln(rows=rows) is deferred, rows
        # history states and a caller's own sequence layout are the seven-launch layer's at every row count
        assert enc.serves_deferred_ln(history=[object()], rows=rows) is False, rows
        assert enc.serves_deferred_ln(seq=object(), rows=rows) is False, rows
        assert enc.serves_deferred_ln(history=[object()], seq=object(), rows=rows) is False, rows
    enc.deferred_ln = False
    for rows, _ in ROWS:
        assert enc.serves_deferred_ln(rows=rows) is False, rows
    enc.deferred_ln = True
    assert enc.serves_deferred_ln(rows=2800) is True
    for flag in ("output_attentions", "output_hidden_states"):    # per-layer outputs: the seven-launch layer writes them
        e = _encoder(width, **{flag: True})
        assert getattr(e, flag) is True
        for rows, _ in ROWS:
            assert e.serves_deferred_ln(rows=rows) is False, (flag, rows)
    both = _encoder(width, output_attentions=True, output_hidden_states=True)
    assert both.serves_deferred_ln(rows=4088) is False and both.serves_deferred_ln() is False


@pytest.mark.parametrize("width", [128, 768])
def test_a_threshold_of_zero_sends_every_row_count_to_the_deferred_loop(width):
    """What the test session's VT_DEFERRED_LN_MIN_ROWS=0 does -- and why a test of the shipped route sets the attribute."""
    enc = _encoder(width)
    enc.deferred_ln_min_rows = 0
    for rows, _ in ROWS:
        assert enc.serves_deferred_ln(rows=rows) is True, rows
        assert enc.serves_deferred_ln(history=[object()], rows=rows) is False, rows


def test_the_constructor_default_is_the_module_constant(monkeypatch):
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT, CaptionBertEncoder

    monkeypatch.delenv("VT_DEFERRED_LN_MIN_ROWS", raising=False)
    assert CaptionBertEncoder(mini_config()).deferred_ln_min_rows == DEFERRED_LN_MIN_ROWS_DEFAULT
    monkeypatch.setenv("VT_DEFERRED_LN_MIN_ROWS", "123")
    assert CaptionBertEncoder(mini_config()).deferred_ln_min_rows == 123
