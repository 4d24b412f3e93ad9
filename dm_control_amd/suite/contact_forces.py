"""Contact-force observations for the device-resident environments: `wrap(env, targets, ...)`.

The twin of `suite/proximity.py` for `contacts.BatchContacts`: where the reference adds `<touch>` sensors to the model or
loops over `mjData.contact` with `mj_contactForce` on the host, the wrapper enqueues one `BatchContacts.net_all()` launch
on the environment's stream after every step and reset and returns, as or in the observation, per target

  quantity='force':   the net contact force, (B, 3 T)
  quantity='normal':  the summed normal force (a touch sensor's reading), (B, T)
  quantity='wrench':  force and torque about `about`, (B, 6 T), per target (force, torque)

in the batch precision.  Nothing is read back to the host and the model is not edited.  `scale='tanh'` squashes on the
device: tanh(x / scale_force), scale_force in newtons (default 100).

refresh=True enqueues `BatchContacts.refresh()` -- one forward launch that leaves the solver's warm start alone -- before
each read: an environment whose control step ends in a plain legacy step leaves a contact list that is newer than its
forces.  refresh=False is for environments whose control step already ends in the forward (`composer.make`).
"""
from dm_control_amd import contacts as contacts_lib
from dm_control_amd.suite import observation_wrapper

_SCALES = (None, 'tanh')
QUANTITIES = ('force', 'normal', 'wrench')


class ContactForceEnv(observation_wrapper.ObservationWrapper):
  """An environment whose observations are (or include) net contact forces; everything else is the wrapped environment's."""
  _ONLY = 'contact_only'

  def __init__(self, env, targets, observation_key='contact_force', contact_only=False, quantity='force', local=False, scale=None,
               refresh=True, about='com', scale_force=100.0):
    if scale not in _SCALES:
      raise ValueError('scale must be one of %s' % (_SCALES,))
    if quantity not in QUANTITIES:
      raise ValueError('quantity must be one of %s' % (QUANTITIES,))
    if scale == 'tanh' and not float(scale_force) > 0:
      raise ValueError("scale='tanh' divides by scale_force: give a positive one")
    super().__init__(env, observation_key, contact_only)
    self.quantity, self.scale, self.scale_force, self.refresh = quantity, scale, float(scale_force), bool(refresh)
    self.contacts = contacts_lib.BatchContacts(env, targets, about=about, local=local)
    self._require_outputs(self.contacts)

  def read(self):
    """The observation of the state in device memory, enqueued on the current stream."""
    import torch      # pylint: disable=import-outside-toplevel
    bc = self.contacts
    if self.refresh:
      bc.refresh()
    if self.quantity == 'normal':
      value = bc.normal()
    else:
      force, torque = bc.net()
      value = force if self.quantity == 'force' else torch.cat([force, torque], dim=-1)
      value = value.reshape(value.shape[0], -1)
    if self.scale == 'tanh':
      value = torch.tanh(value / self.scale_force)
    return value

  def _read(self):
    return self.read()


def wrap(env, targets, observation_key='contact_force', contact_only=False, quantity='force', local=False, scale=None, refresh=True,
         **kw):
  """env: a `fused_env` / `torch_env` / `device_env` / `composer.make` environment; targets: a list of
  `contacts.BatchContacts` targets (a geom name, dict(geom=..), dict(body=..[, subtree=True]), each with other=..).
  kw: about ('com' | 'origin' | 'world'), scale_force."""
  return ContactForceEnv(env, targets, observation_key, contact_only, quantity, local, scale, refresh, **kw)
