"""``jaxsim.api.data`` mirror (``src/jaxsim/api/data.py``)."""

from ..data import (  # noqa: F401
    CONTACT_FIELDS,
    CONTACT_ROWS,
    CONTACT_TIMER_ROWS,
    DONE_TERMINATED,
    DONE_TRUNCATED,
    EVAL_INNERS,
    EVAL_KINDS,
    EVAL_OUTERS,
    ActionSpec,
    ContactSensorSpec,
    JaxSimModelData,
    ObservationSpec,
    RandomStateDistribution,
    RewardSpec,
    random_model_data,
    random_model_data_device,
    random_state_bounds,
)
