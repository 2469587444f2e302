"""CPU: PretrainEngine's precision argument is validated before anything is allocated."""
import pytest


def test_unknown_precision_is_refused_before_allocation():
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.training import PretrainEngine

    model = PreTrainOscar(mini_config())   # on the CPU: an engine that got as far as allocating would refuse it differently
    for bad in ("fp16", "FP32", None, 32):
        with pytest.raises(ValueError):
            PretrainEngine(model, precision=bad)
