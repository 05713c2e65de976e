// poison_switch.h -- host only: the test switch SISIC_POISON_ALLOC (workspace.h says what it does).  Its one read is in
// conv_plan.cpp, next to the dispatch switches; this declaration is all that conv_winograd.hip's scratch growth needs of it.
#pragma once

namespace sisic {

bool poison_alloc();      // SISIC_POISON_ALLOC=1: off unless set, read once per process

}  // namespace sisic
