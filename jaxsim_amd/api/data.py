"""``jaxsim.api.data`` mirror (``src/jaxsim/api/data.py``)."""

from ..data import (  # noqa: F401
    DONE_TERMINATED,
    DONE_TRUNCATED,
    EVAL_INNERS,
    EVAL_KINDS,
    EVAL_OUTERS,
    ActionSpec,
    JaxSimModelData,
    ObservationSpec,
    RandomStateDistribution,
    RewardSpec,
    random_model_data,
    random_model_data_device,
    random_state_bounds,
)
