"""The three value types of the CARLA Python API a walker pose is made of: ``Location``, ``Rotation``, ``Transform``.

When the ``carla`` package imports, these names ARE its classes, so what ``CarlaPose`` builds can be handed to a walker's
``set_bones`` / ``set_transform`` as it is. Without it (no simulator on the machine: every test and every training box) they are
plain value classes with the same constructor keywords and attributes -- metres for the location, degrees for
(pitch, yaw, roll) -- and nothing of the simulator's behaviour: no ``transform()``, no vectors, no world.
"""
try:
    import carla as _carla
    Location, Rotation, Transform = _carla.Location, _carla.Rotation, _carla.Transform
    IS_MOCK = False
except ImportError:
    IS_MOCK = True

    class _Value:
        _fields = ()

        def __eq__(self, other):
            return type(other) is type(self) and all(getattr(self, f) == getattr(other, f) for f in self._fields)

        def __ne__(self, other):
            return not self == other

        __hash__ = None

        def __repr__(self):
            return f'{type(self).__name__}(' + ', '.join(f'{f}={getattr(self, f)!r}' for f in self._fields) + ')'

    class Location(_Value):
        _fields = ('x', 'y', 'z')

        def __init__(self, x=0.0, y=0.0, z=0.0):
            self.x, self.y, self.z = float(x), float(y), float(z)

    class Rotation(_Value):
        _fields = ('pitch', 'yaw', 'roll')

        def __init__(self, pitch=0.0, yaw=0.0, roll=0.0):
            self.pitch, self.yaw, self.roll = float(pitch), float(yaw), float(roll)

    class Transform(_Value):
        _fields = ('location', 'rotation')

        def __init__(self, location=None, rotation=None):
            self.location = location if location is not None else Location()
            self.rotation = rotation if rotation is not None else Rotation()
