"""``jaxsim.api.data`` mirror (``src/jaxsim/api/data.py``)."""

from ..data import (  # noqa: F401
    ActionSpec,
    JaxSimModelData,
    ObservationSpec,
    RandomStateDistribution,
    random_model_data,
    random_model_data_device,
    random_state_bounds,
)
