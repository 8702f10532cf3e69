"""Namespace mirroring ``jaxsim.api`` for the step path: ``import jaxsim_amd.api as js``
then ``js.model.step(model, data)``, ``js.data.JaxSimModelData.build(...)``,
``js.contact.estimate_good_contact_parameters(...)``, ``js.ode.system_dynamics(model, data)``,
``js.com.centroidal_momentum(model, data)``, ``js.link.bias_acceleration(model, data, link_index=...)``,
``js.frame.transform(model, data, frame_index=...)``, ``js.joint.position_limits(model)``."""

from . import com, contact, data, frame, joint, link, model, ode, references  # noqa: F401
