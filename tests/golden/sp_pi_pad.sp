* resistive pi attenuator between unequal ports (50 and 75 ohm): reciprocal, frequency-independent
V1 in 0 DC 0 AC 1 PORTNUM 1 Z0 50
V2 out 0 DC 0 PORTNUM 2 Z0 75
R1 in 0 150
R2 in out 39
R3 out 0 220
.SP LIN 3 1meg 3meg
