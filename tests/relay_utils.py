"""Shared by the relay tests: the ranks of a relay job played one after the other in one process."""


class MailboxComm:
    """RelayComm stand-in for ranks played one after the other in ONE process (the hosts of a single relay trajectory follow
    the rank order, so every state is in the box before its receiver runs); the transport itself -- torch.distributed send /
    recv with the store handshake -- is covered by tests/test_distributed_cpu.py."""

    def __init__(self, box):
        self.box = box

    def send(self, task, state):
        self.box[(task.unit, task.w_end)] = state.clone()

    def ready(self, task, like):
        return (task.unit, task.w_begin) in self.box

    def recv(self, task, like):
        return self.box.pop((task.unit, task.w_begin))

    def finish(self):
        pass
