class DisabledPedestrianWriter(object):
    """``PedestrianWriter``'s interface, doing nothing (reference disabled_pedestrian_writer.py)."""
    reduced_log_every_n_steps = 0

    def __init__(self, *args, **kwargs):
        pass

    def wants(self, step: int, force: bool = False) -> bool:
        return False

    def log_videos(self, *args, **kwargs):
        pass
